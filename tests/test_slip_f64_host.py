"""The float64 slip decision of caller-supplied uniforms (csrc/soccer_slip.hpp: slip_decide4_f64, which
step_kernel_swar<.., SLIPM = 3, ..> expands in place) against the oracle, on the CPU.  For every (tuple, joint action) list of
the reference's transition relation (Oracle.dump_table), uniforms are placed on the list's own SEQUENTIAL float64 running sums
S_k, one ulp either side, on both sides of the 2^-40 margin, inside every entry, and on special values (signed zeros,
subnormals, 1, beyond 1, NaN, infinities).  Each 4-lane group then goes through the decision and the byte-parallel step
(tests/host/swar_host.cpp: swar_step_f64_host) and:
  (a) every lane of every group the decision keeps (not listed) equals the oracle: obs, final_obs, reward, terminated,
      truncated, prob_code and the next state;
  (b) every lane within 2^-41 of an S_k of its list, or at / beyond the list's nominal total, lists its group (the kernel
      then leaves it to the per-lane kernel's exact walk);
  (c) the reference's sums stay within 2^-44 of the nominal thresholds the decision compares with — the claim the 2^-40
      margin rests on — over every list of every slip swept, extreme ones included."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from oracle.oracle import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_STEPS = 100
CLS = (0, 1, 1, 2, 2, 3, 3, 3, 3)        # weight class of slip combination c (reference :211-222)
SPECIALS = np.array([0.0, -0.0, 5e-324, 1.0 - 2.0 ** -53, 1.0, 1.0 + 2.0 ** -52, 7.0, -0.5, np.nan, np.inf, -np.inf])
MARGIN = 2.0 ** -40

# pitch, slip_prob, lists per (tuple, action) kept (None: all)
CASES = [(5, 4, 0.2, None)]
CASES += [(5, 4, s, None) for s in (0.05, 0.1, 0.25, 0.3, 0.5, 0.9, 1.0)]
CASES += [(5, 4, float(s), 1500) for s in np.random.default_rng(20261016).uniform(0.0, 1.0, 30)]
CASES += [(5, 4, s, None) for s in (1e-9, 1e-170, 1.0 - 2.0 ** -30, 1.0 - 1e-12, 0.5 + 2.0 ** -40, 1.0 / 3.0)]
CASES += [(7, 5, s, 4000) for s in (0.2, 0.75, 1.0 / 3.0)] + [(11, 7, s, 4000) for s in (0.1, 0.9)]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("slipf64") / "libswar_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror", "-o", so,
                           os.path.join(ROOT, "tests", "host", "swar_host.cpp")])
    L = C.CDLL(so)
    L.swar_step_f64_host.restype = C.c_int
    L.swar_step_f64_host.argtypes = [C.c_int] * 4 + [C.c_long] + [C.c_void_p] * 11 + [C.c_double] + [C.c_void_p] * 8
    L.swar_slip_f64.argtypes = [C.c_double] + [C.c_void_p] * 4
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def slip_f64(L, slip):
    B = np.zeros(9); w = np.zeros(4); nb = C.c_uint32(); ap = C.c_ulonglong()
    L.swar_slip_f64(float(slip), _p(B), _p(w), C.byref(nb), C.byref(ap))
    return B, w, int(nb.value), [(int(ap.value) >> (4 * i)) & 0xF for i in range(int(nb.value))]


def lists_of(o):
    """(tuple int64[nl, 5], aa, ab, padded probabilities float64[nl, 36], entry count m[nl]) of every (tuple, joint action)"""
    rows, prob = o.dump_table()
    key = rows[:, :7].astype(np.int64)
    start = np.flatnonzero(np.r_[True, np.any(key[1:] != key[:-1], axis=1)])
    m = np.diff(np.r_[start, len(rows)])
    P = np.zeros((len(start), int(m.max())))
    for k in range(int(m.max())):
        sel = m > k
        P[sel, k] = prob[start[sel] + k]
        assert np.all(rows[start[sel] + k, 7] == k)
    return key[start, :5], key[start, 5], key[start, 6], P, m


def nominal_thresholds(row, m, B, w, act):
    """what slip_decide4_f64 compares entry k's running sum with: the end of its combination B[i], or a quarter point
    S0 + q, + q, + q (q = weight / 4, S0 the previous combination's end) — computed in float64 in the kernel's order"""
    out, k = [], 0
    for i, c in enumerate(act):
        W = w[CLS[c]]
        n = {W: 1, W * 0.5: 2, W * 0.25: 4}[row[k]]
        assert all(row[k + j] == row[k] for j in range(n))
        S0 = B[i - 1] if i else 0.0
        q = W * 0.25
        t1 = S0 + q; t2 = t1 + q; t3 = t2 + q
        out += [B[i]] if n == 1 else ([t2, B[i]] if n == 2 else [t1, t2, t3, B[i]])
        k += n
    assert k == m
    return np.array(out)


def candidates(S, m):
    """uniforms for one list with sequential running sums S[:m]; kind labels keep the 4-lane groups homogeneous"""
    s = S[:m]
    lo = np.r_[0.0, s[:-1]]
    cols = [s, np.nextafter(s, 0.0), np.nextafter(s, 2.0)]
    cols += [s + sg * MARGIN * (1 + e * 2.0 ** -20) for sg in (1, -1) for e in (1, -1)]
    cols += [lo + (s - lo) * f for f in (0.25, 0.5, 0.75)]            # inside every entry
    u = np.concatenate(cols + [SPECIALS])
    kind = np.concatenate([np.full(m, j) for j in range(len(cols))] + [len(cols) + np.arange(len(SPECIALS))])
    return u, kind


def run_case(L, w_, h_, slip, keep, rng, autoreset=True, philox_reset=False):
    o = Oracle(w_, h_, slip, n=1, max_steps=MAX_STEPS)
    tup, aa, ab, P, m = lists_of(o)
    B, w, nb, act = slip_f64(L, slip)
    if keep is not None and len(m) > keep:
        sel = np.sort(rng.choice(len(m), keep, replace=False))
        tup, aa, ab, P, m = tup[sel], aa[sel], ab[sel], P[sel], m[sel]
    # one sequential float64 running sum per distinct list (np.add.accumulate adds left to right, as categorical_sample)
    rows, inv = np.unique(P, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    worst = 0.0
    per_row = []
    for r, row in enumerate(rows):
        mr = int(np.count_nonzero(row))
        S = np.add.accumulate(row[:mr])
        worst = max(worst, float(np.max(np.abs(S - nominal_thresholds(row, mr, B, w, act)))))
        per_row.append((S, candidates(S, mr)))
    # lanes: every candidate of every list, ordered by kind so that a group holds one kind of value
    li, ui, ki = [], [], []
    for r, (S, (u, kind)) in enumerate(per_row):
        ls = np.flatnonzero(inv == r)
        li.append(np.repeat(ls, len(u))); ui.append(np.tile(u, len(ls))); ki.append(np.tile(kind, len(ls)))
    li, ui, ki = np.concatenate(li), np.concatenate(ui), np.concatenate(ki)
    order = np.lexsort((li, ki))
    li, ui = li[order], ui[order]
    pad = (-len(li)) % 4
    li = np.r_[li, li[:pad]]; ui = np.r_[ui, ui[:pad]]
    n = len(li)
    st = tup[li]
    t = rng.choice(np.array([0, 1, MAX_STEPS // 2, MAX_STEPS - 2, MAX_STEPS - 1], np.uint8), n)
    a = aa[li].astype(np.uint8); b = ab[li].astype(np.uint8)
    words = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    ur = None if philox_reset else rng.random(n)
    # the oracle: the reference's walk over the same lists
    orc = Oracle(w_, h_, slip, n=n, max_steps=MAX_STEPS, autoreset=autoreset)
    orc.set_state(st[:, 0], st[:, 1], st[:, 2], st[:, 3], st[:, 4], t=t, needs_reset=np.zeros(n, np.uint8))
    ref = orc.step(a.view(np.int8), b.view(np.int8), u_step=ui,
                   u_reset=((words & 3).astype(np.float64) + 0.5) * 0.25 if philox_reset else ur)
    # the decision + the byte-parallel step
    ra, ca, rb, cb = (np.ascontiguousarray(st[:, k], np.uint8) for k in range(4))
    ps = np.ascontiguousarray(st[:, 4], np.uint8); tt = t.copy()
    out = {k: np.zeros(n, np.uint16) for k in ("obs", "final_obs")}
    out.update({k: np.zeros(n, np.uint8) for k in ("reward", "terminated", "truncated", "prob_code", "frozen")})
    listed = np.zeros(n // 4, np.uint8)
    rc = L.swar_step_f64_host(w_, h_, MAX_STEPS, int(autoreset), n, _p(ra), _p(ca), _p(rb), _p(cb), _p(ps), _p(tt),
                              _p(a), _p(b), _p(np.ascontiguousarray(ui)), _p(ur), _p(words), float(slip),
                              _p(out["obs"]), _p(out["final_obs"]), _p(out["reward"]), _p(out["terminated"]),
                              _p(out["truncated"]), _p(out["prob_code"]), _p(out["frozen"]), _p(listed))
    assert rc == 0
    lane_listed = np.repeat(listed.astype(bool), 4)
    keep_ = ~lane_listed
    what = "%dx%d slip %r" % (w_, h_, slip)
    assert keep_.any(), what + ": the decision kept nothing"         # (near slip 0 or 1 most entries are inside the margin)
    # (a) the kept groups are the reference's, lane by lane
    for k, got in (("obs", out["obs"]), ("final_obs", out["final_obs"]), ("reward", out["reward"].view(np.int8)),
                   ("terminated", out["terminated"]), ("truncated", out["truncated"]), ("prob_code", out["prob_code"])):
        bad = np.flatnonzero(keep_ & (got != ref[k]))
        assert bad.size == 0, "%s: %s differs on %d kept lanes, e.g. u=%r list %d" % (what, k, bad.size, ui[bad[0]], li[bad[0]])
    for got, exp, k in ((ra, orc.row_a, "row_a"), (ca, orc.col_a, "col_a"), (rb, orc.row_b, "row_b"), (cb, orc.col_b, "col_b"),
                        (ps, orc.poss, "poss"), (tt, orc.t, "t")):
        bad = np.flatnonzero(keep_ & (got != exp.view(np.uint8)))
        assert bad.size == 0, "%s: next %s differs on %d kept lanes, e.g. u=%r" % (what, k, bad.size, ui[bad[0]])
    assert not np.any(out["frozen"][keep_])
    # (b) every lane within 2^-41 of one of its list's running sums, or at / beyond the nominal total, is listed
    must = ui >= B[nb - 1]
    for r, (S, _) in enumerate(per_row):
        lanes = np.flatnonzero(inv[li] == r)
        d = np.min(np.abs(ui[lanes, None] - S[None, :]), axis=1)
        must[lanes] |= d < 2.0 ** -41
    bad = np.flatnonzero(must & ~lane_listed)
    assert bad.size == 0, "%s: %d lanes next to a running sum or beyond the total were not listed, e.g. u=%r" % (what, bad.size, ui[bad[0]])
    assert lane_listed.any()
    return worst, int(listed.sum()), n


def test_slip_f64_decision_against_the_reference_lists(host):
    rng = np.random.default_rng(7)
    worst, report = 0.0, []
    for (w_, h_, slip, keep) in CASES:
        d, nl, n = run_case(host, w_, h_, slip, keep, rng)
        worst = max(worst, d)
        report.append("%dx%d slip %-22r listed %6d of %7d groups, max |S - nominal| = %.3g" % (w_, h_, slip, nl, n // 4, d))
    print("\n".join(report))
    print("max |reference running sum - nominal threshold| over every list swept: %.3g = 2^%.1f"
          % (worst, math.log2(worst) if worst > 0 else float("-inf")))
    # (c) the margin the kernel relies on: the reference's sums stay far inside 2^-40 of the nominal thresholds
    assert worst < 2.0 ** -44


@pytest.mark.parametrize("w_,h_,slip", [(5, 4, 0.2), (7, 5, 0.3), (5, 4, 1.0)])
def test_slip_f64_decision_with_philox_reset_draws(host, w_, h_, slip):
    """u_reset NULL: the reset draw of a lane whose episode ends comes from its Philox word (w & 3), next to caller step uniforms"""
    run_case(host, w_, h_, slip, 3000, np.random.default_rng(11), philox_reset=True)


@pytest.mark.parametrize("w_,h_,slip", [(5, 4, 0.2), (9, 6, 0.1)])
def test_slip_f64_decision_without_autoreset(host, w_, h_, slip):
    """autoreset off: a finished lane keeps its end tuple and the needs-reset flag (the general step4 instantiation)"""
    run_case(host, w_, h_, slip, 3000, np.random.default_rng(13), autoreset=False)
