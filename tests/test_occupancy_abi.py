"""CPU-side checks of soccer_occupancy's place in the C ABI: the symbol is exported, declared and mirrored, nothing that
existed changed, and the call checks its handle before anything else, whatever else it is given."""
import os
import re

import numpy as np
import pytest

from gym_soccer_littman94_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THETA, C_PROB = 1e-10, 0.9


def test_the_symbol_is_declared_exported_and_mirrored():
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "soccer_hip.h")).read()
    assert hasattr(lib, "soccer_occupancy"), "libsoccer_hip.so does not export soccer_occupancy"
    assert re.search(r"\bint soccer_occupancy\(", text), "soccer_occupancy is not declared"
    assert "soccer_occupancy" in _lib.PROTOTYPES
    restype, args = _lib.PROTOTYPES["soccer_occupancy"]
    # the handle, n_a, pi_a, n_b, pi_b, theta, continue_prob, max_sweeps, pairs_per_pass, n_f, features, and the four outputs
    assert len(args) == 15 and len(re.search(r"int soccer_occupancy\((.*?)\);", text, re.S).group(1).split(",")) == 15
    assert text.index("---- match outcomes") < text.index("---- state occupancy") < text.index("---- the meta-game")
    assert text.index("---- state occupancy") < text.index("int soccer_occupancy(") < text.index("---- the meta-game")
    assert "soccer_occupancy" in re.search(r"#define SOCCER_ABI_VERSION 3.*?\*/", text, re.S).group(0)
    assert re.search(r"#define SOCCER_OCC_MAX_FEATURES 16\b", text) and _lib.OCC_MAX_FEATURES == 16
    assert lib.soccer_abi_version() == 3          # nothing that existed changed
    assert re.search(r"#define SOCCER_ABI_VERSION 3\b", text)


@pytest.mark.parametrize("n_a,n_b,theta,c,sweeps,ppp,n_f", [
    (1, 1, THETA, C_PROB, 10, 0, 1), (0, 1, THETA, C_PROB, 10, 0, 1), (1, 1025, THETA, C_PROB, 10, 0, 1), (1, 1, -1.0, C_PROB, 10, 0, 1),
    (1, 1, THETA, 1.5, 10, 0, 1), (1, 1, THETA, C_PROB, 0, 0, 1), (1, 1, THETA, C_PROB, 10, 63, 1), (1, 1, THETA, C_PROB, 10, 0, 17)])
def test_the_call_rejects_a_null_handle_before_any_output_is_touched(n_a, n_b, theta, c, sweeps, ppp, n_f):
    lib = _lib.load()
    pol = np.full((1, 761, 5), 0.2)
    feat = np.ones((17, 761))
    length = np.full(1, 7.0); expect = np.full(17, 7.0); occ = np.full(761, 7.0)
    it = np.full(1, 7, np.int32)
    assert lib.soccer_occupancy(None, n_a, pol.ctypes.data, n_b, pol.ctypes.data, theta, c, sweeps, ppp, n_f, feat.ctypes.data,
                                length.ctypes.data, expect.ctypes.data, occ.ctypes.data, it.ctypes.data) == _lib.E_INVALID
    assert b"handle is NULL" in lib.soccer_last_error(None)
    assert length[0] == 7.0 and (expect == 7.0).all() and (occ == 7.0).all() and it[0] == 7


def test_null_outputs_and_null_policies_are_no_way_past_the_handle_check():
    lib = _lib.load()
    assert lib.soccer_occupancy(None, 1, None, 1, None, THETA, C_PROB, 10, 0, 0, None, None, None, None, None) == _lib.E_INVALID
    assert b"handle is NULL" in lib.soccer_last_error(None)
