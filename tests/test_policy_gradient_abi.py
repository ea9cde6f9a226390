"""CPU-side checks of soccer_policy_gradient's and soccer_gradient_play_*'s place in the C ABI: the symbols are exported,
declared in order and mirrored with the right number of arguments, nothing that existed changed, and the calls check their
handle before anything else, whatever else they are given."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gym_soccer_littman94_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THETA, GAMMA = 1e-10, 0.9
# name -> the number of arguments, in the order of their declarations
SYMBOLS = [("soccer_policy_gradient", 22), ("soccer_gradient_play_create", 3), ("soccer_gradient_play_destroy", 2),
           ("soccer_gradient_play_run", 4), ("soccer_gradient_play_read", 10), ("soccer_gradient_play_load", 8),
           ("soccer_gradient_play_set_weights", 4)]


def test_the_symbols_are_declared_in_order_exported_and_mirrored():
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "soccer_hip.h")).read()
    at = text.index("---- state occupancy")
    assert at < text.index("int soccer_occupancy(") < text.index("---- exact policy gradients") < text.index("---- the meta-game")
    at = text.index("---- exact policy gradients")
    for name, n_args in SYMBOLS:
        assert hasattr(lib, name), "libsoccer_hip.so does not export %s" % name
        m = re.search(r"\bint %s\((.*?)\);" % name, text, re.S)
        assert m, "%s is not declared" % name
        assert at < m.start() < text.index("---- the meta-game"), "%s is declared out of order" % name
        at = m.start()
        assert len(m.group(1).split(",")) == n_args, name
        restype, args = _lib.PROTOTYPES[name]
        assert restype is C.c_int and len(args) == n_args, name
    version = re.search(r"#define SOCCER_ABI_VERSION 3.*?\*/", text, re.S).group(0)
    assert "soccer_policy_gradient" in version and "soccer_gradient_play_*" in version
    assert lib.soccer_abi_version() == 3          # nothing that existed changed
    assert re.search(r"#define SOCCER_ABI_VERSION 3\b", text)
    # the config is mirrored field for field
    body = re.search(r"typedef struct soccer_gradient_play_config \{(.*?)\} soccer_gradient_play_config;", text, re.S).group(1)
    names = [n.strip(" *\n") for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") if decl.strip()
             for n in decl.replace("const double*", "").replace("int32_t", "").replace("double", "").split(",")]
    assert names == [f[0] for f in _lib.GradientPlayConfig._fields_]
    assert C.sizeof(_lib.GradientPlayConfig) == 80


@pytest.mark.parametrize("n_a,n_b,theta,gamma,sweeps,ppp", [
    (1, 1, THETA, GAMMA, 10, 0), (0, 1, THETA, GAMMA, 10, 0), (1, 1025, THETA, GAMMA, 10, 0), (1, 1, -1.0, GAMMA, 10, 0),
    (1, 1, THETA, 1.5, 10, 0), (1, 1, THETA, GAMMA, 0, 0), (1, 1, THETA, GAMMA, 10, 63)])
def test_the_call_rejects_a_null_handle_before_any_output_is_touched(n_a, n_b, theta, gamma, sweeps, ppp):
    lib = _lib.load()
    pol = np.full((1, 761, 5), 0.2)
    w = np.array([float("nan")])
    outs = [np.full(n, 7.0) for n in (1, 3805, 3805, 761, 761, 3805, 3805, 761, 761)]
    it = np.full(2, 7, np.int32)
    assert lib.soccer_policy_gradient(None, n_a, pol.ctypes.data, n_b, pol.ctypes.data, theta, gamma, sweeps, ppp, w.ctypes.data,
                                      w.ctypes.data, 1, *[o.ctypes.data for o in outs], it.ctypes.data) == _lib.E_INVALID
    assert b"handle is NULL" in lib.soccer_last_error(None)
    assert all((o == 7.0).all() for o in outs) and (it == 7).all()


def test_null_arguments_are_no_way_past_the_handle_check():
    lib = _lib.load()
    assert lib.soccer_policy_gradient(None, 1, None, 1, None, THETA, GAMMA, 10, 0, None, None, 0, *[None] * 10) == _lib.E_INVALID
    assert b"handle is NULL" in lib.soccer_last_error(None)
    out = C.c_void_p(7)
    cfg = _lib.GradientPlayConfig(1, 1, 1.0, 1.0, 0.0, GAMMA, THETA, 0, 10, 0, 0, None, None)
    assert lib.soccer_gradient_play_create(None, C.byref(cfg), C.byref(out)) == _lib.E_INVALID and out.value == 7
    assert b"handle is NULL" in lib.soccer_last_error(None)
    trace = np.full(4, 7.0); steps = C.c_int64(7)
    assert lib.soccer_gradient_play_run(None, None, 4, trace.ctypes.data) == _lib.E_INVALID and (trace == 7.0).all()
    assert lib.soccer_gradient_play_read(None, None, *[None] * 7, C.byref(steps)) == _lib.E_INVALID and steps.value == 7
    assert lib.soccer_gradient_play_load(None, None, *[None] * 5, C.byref(steps)) == _lib.E_INVALID
    assert lib.soccer_gradient_play_set_weights(None, None, None, None) == _lib.E_INVALID
    assert lib.soccer_gradient_play_destroy(None, None) == _lib.E_INVALID
    assert b"handle is NULL" in lib.soccer_last_error(None)
