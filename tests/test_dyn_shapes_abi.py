"""The runtime-shaped kernel family at the C boundary, without a GPU: the two new constants, the limits and their
messages (every refusal happens before any device work), the rollout selection's new value, the runner's keyword."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _define(header, name):
    with open(os.path.join(ROOT, "include", header)) as f:
        m = re.search(r"^#define %s (\d+)\b" % name, f.read(), flags=re.M)
    assert m, "%s is not defined in %s" % (name, header)
    return int(m.group(1))


def test_constants_match_the_headers():
    from fdr import _lib
    assert _lib.FDR_ROLLOUT_GENERIC == _define("fdr.h", "FDR_ROLLOUT_GENERIC") == 4
    assert _lib.FDR_LOADER_DYN == _define("fdr_diag.h", "FDR_LOADER_DYN") == 2
    codes = [_define("fdr.h", "FDR_ROLLOUT_" + n) for n in ("PAIR", "SINGLE", "AUTO", "WIDE", "GENERIC")]
    assert sorted(codes) == [0, 1, 2, 3, 4]
    assert _lib.lib.fdr_version().startswith(b"fdr 0.5")


def _calls(lib, pd):
    """The three entry points that take an MLP policy shape, every pointer argument a dummy: the shape is checked
    first."""
    from fdr import _lib
    ld = _lib.LanesDesc(1, 0, None, 0, None, None, 0.0, None)
    ed = _lib.EnvDesc(_lib.FDR_ENV_SYNTH, pd.n_in, pd.n_act, 10, 1, 1, 1, None, 0, 0, 0.0, 0)
    return {
        "fdr_policy_forward": lambda: lib.fdr_policy_forward(None, ctypes.byref(pd), ctypes.byref(ld), 1, 1, 1, 1, None),
        "fdr_rollout": lambda: lib.fdr_rollout(None, ctypes.byref(pd), ctypes.byref(ed), ctypes.byref(ld), 1,
                                               ctypes.c_uint64(1), 0, None, None, 1, 1, 1, None, None),
        "fdr_diag_theta_prime": lambda: lib.fdr_diag_theta_prime(None, ctypes.byref(pd), ctypes.byref(ld), 1,
                                                                 _lib.FDR_LOADER_DYN, 1, 1, 1, 1, None),
    }


LIMITS = [("discrete", 65, 2, b"n_in must be in 1..64"), ("mujoco", 65, 2, b"n_in must be in 1..64"),
          ("discrete", 0, 2, b"n_in must be in 1..64"), ("discrete", 4, 17, b"n_act must be in 1..16"),
          ("discrete", 4, 0, b"n_act must be in 1..16"), ("mujoco", 4, 9, b"n_act must be in 1..8"),
          ("mujoco", 4, 0, b"n_act must be in 1..8")]


@pytest.mark.parametrize("entry", ["fdr_policy_forward", "fdr_rollout", "fdr_diag_theta_prime"])
@pytest.mark.parametrize("kind,n_in,n_act,text", LIMITS)
def test_shape_limits_without_gpu(entry, kind, n_in, n_act, text):
    """A shape outside the limits is FDR_ERR_UNSUPPORTED with the limit in the message, before any device work."""
    from fdr import _lib
    k = _lib.FDR_POLICY_DISCRETE if kind == "discrete" else _lib.FDR_POLICY_MUJOCO
    pd = _lib.PolicyDesc(k, n_in, n_act, 64, 1000, None, None)
    assert _calls(_lib.lib, pd)[entry]() == _lib.FDR_ERR_UNSUPPORTED
    assert text in _lib.lib.fdr_last_error()


def test_hidden_width_is_still_checked_first():
    from fdr import _lib
    pd = _lib.PolicyDesc(_lib.FDR_POLICY_MUJOCO, 65, 9, 32, 1000, None, None)
    assert _calls(_lib.lib, pd)["fdr_policy_forward"]() == _lib.FDR_ERR_UNSUPPORTED
    assert _lib.lib.fdr_last_error() == b"hidden width must be 64"


@pytest.mark.parametrize("kind,n_in,n_act", [("discrete", 64, 16), ("mujoco", 64, 8), ("discrete", 1, 1),
                                             ("mujoco", 24, 4)])
def test_shapes_within_the_limits_pass_the_shape_check(kind, n_in, n_act):
    """Within the limits the shape check lets the call through to the next one (here: the lanes descriptor's NULL
    base, FDR_ERR_INVALID)."""
    from fdr import _lib
    k = _lib.FDR_POLICY_DISCRETE if kind == "discrete" else _lib.FDR_POLICY_MUJOCO
    pd = _lib.PolicyDesc(k, n_in, n_act, 64, 1000, None, None)
    ld = _lib.LanesDesc(None, 0, None, 0, None, None, 0.0, None)
    rc = _lib.lib.fdr_policy_forward(None, ctypes.byref(pd), ctypes.byref(ld), 1, 1, 1, 1, None)
    assert rc == _lib.FDR_ERR_INVALID
    assert b"base is NULL" in _lib.lib.fdr_last_error()


def test_rollout_selection_accepts_generic():
    from fdr import _lib
    lib = _lib.lib
    names = {"pair": _lib.FDR_ROLLOUT_PAIR, "single": _lib.FDR_ROLLOUT_SINGLE, "wide": _lib.FDR_ROLLOUT_WIDE,
             "generic": _lib.FDR_ROLLOUT_GENERIC}
    restore = names.get(os.environ.get("FDR_ROLLOUT"), _lib.FDR_ROLLOUT_AUTO)
    try:
        assert lib.fdr_ctx_set_rollout_impl(None, _lib.FDR_ROLLOUT_GENERIC) == _lib.FDR_OK
        assert lib.fdr_rollout_set_impl(_lib.FDR_ROLLOUT_GENERIC) == _lib.FDR_OK
        assert lib.fdr_rollout_set_impl(5) == _lib.FDR_ERR_INVALID
        assert lib.fdr_rollout_set_impl(-1) == _lib.FDR_ERR_INVALID
    finally:
        assert lib.fdr_rollout_set_impl(restore) == _lib.FDR_OK


def test_unknown_loader_is_still_invalid():
    from fdr import _lib
    pd = _lib.PolicyDesc(_lib.FDR_POLICY_MUJOCO, 17, 6, 64, 6092, None, None)
    ld = _lib.LanesDesc(1, 0, None, 0, None, None, 0.0, None)
    rc = _lib.lib.fdr_diag_theta_prime(None, ctypes.byref(pd), ctypes.byref(ld), 1, 3, 1, 1, 1, 1, None)
    assert rc == _lib.FDR_ERR_INVALID and _lib.lib.fdr_last_error() == b"unknown loader"


def test_engine_and_runner_expose_the_new_names():
    from fdr import engine
    from run_sequential import SequentialRunner
    assert "generic" in inspect.getsource(engine.Context.set_rollout_impl)
    assert '"dyn"' in inspect.getsource(engine.theta_prime)
    p = inspect.signature(SequentialRunner.__init__).parameters
    assert "env_shape" in p and p["env_shape"].default is None
