"""CPU: the in-list builder of soccer_occupancy (csrc/soccer_inlists.hpp) run by a stand-alone host program
(tests/host/inlists_host.cpp, built with AddressSanitizer and UndefinedBehaviorSanitizer) on a small hand-made out-list and on
the oracle's lists of 5x4, and of 6x5, 7x5 at slip 1 and 8x7 without slip — the three shapes the in-lists take, 344, 152 and 40
entries at the longest — against tests/occupancy_np.py's in_lists integer for integer: entries that end the game, padding and
source state 0 are dropped, the rest stand by ascending source key and then by position, every in-list padded to four."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle.oracle import Oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import occupancy_np as ocn  # noqa: E402
from minimax_q_np import shapley_lists  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DONE = -(1 << 31)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("inlists_host")), "inlists_host")
    # the sanitizers' runtimes are linked statically: the program runs as it is, with nothing preloaded
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-Wall", "-Wextra", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "host", "inlists_host.cpp")])
    return exe


def run(host, tmp_path, nS, offset, prob, next_done):
    """the program's (status, in_offset, in_prob bits, in_key, pad) on out-lists given as CSR arrays"""
    path = os.path.join(str(tmp_path), "lists.txt")
    pb = np.asarray(prob, np.float64).view(np.uint64)
    with open(path, "w") as f:
        f.write("%d %d\n%s\n" % (nS, len(prob), " ".join(str(int(o)) for o in offset)))
        f.write("\n".join("%d %d" % (int(b), int(n)) for b, n in zip(pb, next_done)) + "\n")
    # (the leak check at exit needs ptrace, which a container may withhold; the checks of every access stay on)
    p = subprocess.run([host, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert p.returncode in (0, 2), p.stderr
    if p.returncode == 2:
        return 2, None, None, None, None
    lines = p.stdout.split("\n")
    off = np.array(lines[0].split(), np.int64)
    ent = np.array([ln.split() for ln in lines[1:] if ln], dtype=np.uint64).reshape(-1, 3)
    return 0, off, ent[:, 0], ent[:, 1].astype(np.int64), ent[:, 2].astype(np.int64)


def restated(nS, offset, prob, next_done):
    offset = np.asarray(offset, np.int64); nd = np.asarray(next_done, np.int64)
    key = np.repeat(np.arange(nS * 25), np.diff(offset))
    off, in_prob, in_key = ocn.in_lists(nS, key, prob, nd & 0x7fffffff, nd < 0)
    return off, in_prob.view(np.uint64), in_key


def hand_made():
    """three states.  Key by key, (prob, next, done): state 0's lists hold live-looking entries that must be dropped for
    their source; state 1 and 2 send entries to each other, to themselves, to state 0 with the done bit, and carry padding
    (prob 0, next 0, done)"""
    lists = {k: [] for k in range(75)}
    lists[0] = [(0.5, 1, False), (0.5, 2, False)]                       # source state 0: dropped
    lists[7] = [(1.0, 1, False)]                                        # ... also this one
    lists[25] = [(0.25, 2, False), (0.5, 1, False), (0.25, 0, True), (0.0, 0, True)]      # (the last: padding)
    lists[26] = [(1.0, 0, True)]
    lists[31] = [(0.125, 2, False), (0.375, 2, False), (0.5, 1, False)]                   # two entries of one key to one state
    lists[49] = [(1.0, 2, False)]
    lists[50] = [(0.75, 1, False), (0.25, 2, True)]                     # (done with a next that is not 0: dropped all the same)
    lists[51] = [(0.0, 1, False)]                                       # a live entry of probability 0 is kept
    lists[74] = [(0.5, 1, False), (0.5, 2, False), (0.0, 0, True), (0.0, 0, True)]
    offset, prob, nd = [0], [], []
    for k in range(75):
        for p, n, d in lists[k]:
            prob.append(p); nd.append(n + (DONE if d else 0))
        offset.append(len(prob))
    return 3, offset, prob, nd


def test_a_hand_made_list(host, tmp_path):
    nS, offset, prob, nd = hand_made()
    status, off, pb, key, pad = run(host, tmp_path, nS, offset, prob, nd)
    assert status == 0
    # spelled out: state 0 is reached by nothing that is kept; state 1 by keys 25, 31, 50, 51, 74; state 2 by 25, 31, 31, 49, 74
    assert off.tolist() == [0, 0, 8, 16]
    assert key.tolist() == [25, 31, 50, 51, 74, 0, 0, 0, 25, 31, 31, 49, 74, 0, 0, 0]
    assert pb.view(np.float64).tolist() == [0.5, 0.5, 0.75, 0.0, 0.5, 0, 0, 0, 0.25, 0.125, 0.375, 1.0, 0.5, 0, 0, 0]
    assert (pad == 0).all() and not np.signbit(pb.view(np.float64)).any()
    # and against numpy, integer for integer
    w_off, w_pb, w_key = restated(nS, offset, prob, nd)
    assert off.tolist() == w_off.tolist() and pb.tolist() == w_pb.tolist() and key.tolist() == w_key.tolist()


def test_a_next_state_past_the_end_is_refused(host, tmp_path):
    nS, offset, prob, nd = hand_made()
    assert offset[25] == 3 and nd[3] == 2       # key 25's first entry, which is kept
    nd[3] = 3
    assert run(host, tmp_path, nS, offset, prob, nd)[0] == 2


def oracle_lists_through_the_program(host, tmp_path, w, h, slip):
    """the program's in-lists of the oracle's lists against numpy's, integer for integer: (in_offset, in_key, the out-lists)"""
    Pp, Pn, Pr, Pd = shapley_lists(Oracle(w, h, slip, n=1, seed=0))
    nS, _, K = Pp.shape
    # CSR with the padded arrays' rows as they are: padding is (prob 0, next 0, done)
    offset = np.arange(nS * 25 + 1) * K
    nd = Pn.reshape(-1) + np.where(Pd.reshape(-1) == 0.0, DONE, 0)
    status, off, pb, key, pad = run(host, tmp_path, nS, offset, Pp.reshape(-1), nd)
    w_off, w_prob, w_key = ocn.in_lists_of((Pp, Pn, Pr, Pd))
    assert status == 0 and off.tolist() == w_off.tolist()
    assert np.array_equal(pb, w_prob.view(np.uint64)) and np.array_equal(key, w_key) and (pad == 0).all()
    size = np.diff(off)
    print("%dx%d at slip %.1f: K %d, %d in-entries with padding, in-lists of %d .. %d" % (w, h, slip, K, off[-1], size.min(), size.max()))
    assert (size % 4 == 0).all() and size[0] == 0 and (key[pb == 0] >= 0).all() and off[-1] == w_prob.size
    live = key[key != 0]
    assert (live >= 25).all() and live.size == int(((Pd != 0) & (np.arange(nS)[:, None, None] != 0)).sum())
    return off, key, (Pp, Pn, Pr, Pd)


def test_the_oracle_s_lists(host, tmp_path):
    oracle_lists_through_the_program(host, tmp_path, 5, 4, 0.2)


@pytest.mark.parametrize("w,h,slip,longest,K", [(6, 5, 0.2, 344, 15), (7, 5, 1.0, 152, 7), (8, 7, 0.0, 40, 4)], ids=["6x5", "7x5_slip1", "8x7_slip0"])
def test_the_oracle_s_lists_of_the_other_in_list_shapes(host, tmp_path, w, h, slip, longest, K):
    """an ordinary slip on an even width, slip 1 (every move may go astray: fewer distinct outcomes a key, K = 7) and no slip on a
    large pitch (K = 4: in-lists of 40 at the longest)"""
    off, key, lists = oracle_lists_through_the_program(host, tmp_path, w, h, slip)
    assert int(np.diff(off).max()) == longest and lists[0].shape[2] == K
    # every state but 0 is reached from somewhere, and the longest in-list is no outlier of one state
    size = np.diff(off)
    assert (size[1:] > 0).all() and (size == longest).sum() > 1
