"""The boundary of the map log and of phd_trajectories_at without a GPU: the four entry points are declared, exported and
refuse a NULL handle with their outputs untouched, and the ctypes wrapper, the loader, the hosts and the scripts carry the new
members."""
import ctypes as C
import inspect
import os
import sys

from monorfs_amd import _lib
from monorfs_amd.abi import PHD_ERR_BAD_ARGUMENT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("phd_map_history_enable", "phd_map_history_append", "phd_map_history", "phd_trajectories_at")


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
    assert lib.phd_map_history_enable(None, 16, 1000) == PHD_ERR_BAD_ARGUMENT
    assert lib.phd_map_history_append(None, 0.0) == PHD_ERR_BAD_ARGUMENT
    n = C.c_int(0)
    t, b, x, cnt, off, w, m, c = _lib.dp(), _lib.ip(), _lib.dp(), _lib.ip(), _lib.i64p(), _lib.dp(), _lib.dp(), _lib.dp()
    assert lib.phd_map_history(None, C.byref(n), C.byref(t), C.byref(b), C.byref(x), C.byref(cnt), C.byref(off), C.byref(w), C.byref(m), C.byref(c)) == PHD_ERR_BAD_ARGUMENT
    assert n.value == 0 and not any((t, b, x, cnt, off, w, m, c))
    q = (C.c_int32 * 1)(0)
    t, x, s = _lib.dp(), _lib.dp(), _lib.ip()
    assert lib.phd_trajectories_at(None, 0, q, 1, C.byref(n), C.byref(t), C.byref(x), C.byref(s)) == PHD_ERR_BAD_ARGUMENT
    assert n.value == 0 and not t and not x and not s


def test_wrapper_hosts_and_scripts_have_the_members():
    from monorfs_amd import navigator
    for m in ("enable_map_history", "append_map_history", "WayMaps", "WayPointsAt"):
        assert callable(getattr(navigator.PHDNavigator, m))
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import replay
    sig = inspect.signature(replay.replay)
    assert list(sig.parameters)[-1] == "posted" and sig.parameters["posted"].default is False
    assert list(sig.parameters)[:4] == ["rec", "particles", "seed", "solver_cls"] and sig.parameters["estimate"].default == "poses"
    hpp = open(os.path.join(ROOT, "monorfs_amd", "host", "PHDNavigator.hpp")).read()
    cs = open(os.path.join(ROOT, "bindings", "csharp", "HipPHDNavigator.cs")).read()
    for n in NAMES:
        assert n in hpp and n in cs, n
    for m in ("enableMapHistory", "appendMapHistory", "WayMaps", "WayPointsAt"):
        assert m in hpp, m
    for m in ("EnableDeviceMapHistory", "AppendDeviceMapHistory", "DeviceWayMaps", "DeviceWayPointsAt"):
        assert m in cs, m
