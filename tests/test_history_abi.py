"""The boundary of the trajectory log without a GPU: the three entry points are declared, exported and refuse a NULL handle,
and the ctypes wrapper, the loader and the scripts carry the new members."""
import ctypes as C
import inspect
import os
import sys

from monorfs_amd import _lib
from monorfs_amd.abi import PHD_ERR_BAD_ARGUMENT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("phd_history_enable", "phd_history_append", "phd_trajectories")


def test_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "phdhip.h")).read()
    lib = C.CDLL(_lib.build())
    for n in NAMES:
        assert n + "(phd_navigator* nav" in header, n
        assert hasattr(lib, n), "libphdhip.so does not export %s" % n
        assert n in _lib.EXPORTS
    assert "#define PHD_API_VERSION 4" in header


def test_null_handle_is_refused():
    lib = _lib.load()
    assert lib.phd_history_enable(None, 16) == PHD_ERR_BAD_ARGUMENT
    assert lib.phd_history_append(None, 0.0) == PHD_ERR_BAD_ARGUMENT
    q = (C.c_int32 * 1)(0)
    n, t, x, s = C.c_int(0), _lib.dp(), _lib.dp(), _lib.ip()
    assert lib.phd_trajectories(None, q, 1, C.byref(n), C.byref(t), C.byref(x), C.byref(s)) != 0
    assert n.value == 0 and not t and not x and not s


def test_wrapper_and_scripts_have_the_members():
    from monorfs_amd import navigator
    for m in ("enable_history", "append_history", "WayPoints"):
        assert callable(getattr(navigator.PHDNavigator, m))
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import replay
    import simulate
    sig = inspect.signature(replay.replay)
    assert list(sig.parameters)[:4] == ["rec", "particles", "seed", "solver_cls"] and sig.parameters["estimate"].default == "poses"
    assert inspect.signature(simulate.simulate).parameters["estimate"].default == "poses"
    hpp = open(os.path.join(ROOT, "monorfs_amd", "host", "PHDNavigator.hpp")).read()
    cs = open(os.path.join(ROOT, "bindings", "csharp", "HipPHDNavigator.cs")).read()
    for n in NAMES:
        assert n in hpp and n in cs, n
