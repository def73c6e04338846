"""The boundary of phd_pose_error without a GPU: the entry point is declared, exported and bound, refuses a NULL handle with its
outputs untouched, and the wrapper, the hosts, the replay script and the documents carry the new members."""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np

from monorfs_amd import _lib
from monorfs_amd.abi import PHD_ERR_BAD_ARGUMENT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "phdhip.h")).read()
    lib = C.CDLL(_lib.build())
    assert "int phd_pose_error(phd_navigator* nav, int mode," in header
    for name, value in (("TIMED", 0), ("SMOOTH", 1), ("FILTER", 2)):
        assert re.search(r"#define PHD_POSE_ERROR_%s\s+%d\b" % (name, value), header), name
    assert hasattr(lib, "phd_pose_error"), "libphdhip.so does not export phd_pose_error"
    assert "phd_pose_error" in _lib.EXPORTS
    assert "phd_poseerror.h" in _lib.SOURCES
    bound = _lib.load().phd_pose_error
    assert bound.restype is C.c_int and len(bound.argtypes) == 16
    assert "#define PHD_API_VERSION 4" in header              # detected by symbol: no version bump
    # the bound the header states is the one the kernel is built for, and holds the ten-minute record of INTEGRATION.md
    kernel = open(os.path.join(ROOT, "monorfs_amd", "csrc", "phd_poseerror.h")).read()
    stated = int(re.search(r"#define PHD_POSE_ERROR_MAX\s+(\d+)", header).group(1))
    assert stated == int(re.search(r"#define PHD_POSEERR_MAX (\d+)", kernel).group(1)) and stated >= 18000


def test_null_handle_is_refused():
    lib = _lib.load()
    n, m = C.c_int(0), C.c_int(0)
    out = [_lib.dp() for _ in range(6)]
    truth = np.array([0, 0, 0, 1.0, 0, 0, 0])
    rc = lib.phd_pose_error(None, 0, truth.ctypes.data_as(_lib.dp), 1, None, 0, 0, 0.0, C.byref(n), C.byref(out[0]), C.byref(out[1]), C.byref(out[2]),
                            C.byref(m), C.byref(out[3]), C.byref(out[4]), C.byref(out[5]))
    assert rc == PHD_ERR_BAD_ARGUMENT
    assert n.value == 0 and m.value == 0 and not any(out)


def test_wrapper_hosts_and_scripts_have_the_members():
    from monorfs_amd import navigator
    sig = inspect.signature(navigator.PHDNavigator.PoseError)
    assert list(sig.parameters) == ["self", "truth", "mode", "slots", "first_entry", "ref_entry", "slam_time"]
    assert [sig.parameters[k].default for k in ("mode", "slots", "first_entry", "ref_entry", "slam_time")] == ["timed", None, 0, 0, 0.0]
    assert navigator.PHDNavigator.POSE_ERROR_MODES == {"timed": 0, "smooth": 1, "filter": 2}
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import replay
    params = inspect.signature(replay.replay).parameters
    assert params["pose_error"].default is None and params["reftime"].default == 0.0
    hpp = open(os.path.join(ROOT, "monorfs_amd", "host", "PHDNavigator.hpp")).read()
    metric = open(os.path.join(ROOT, "monorfs_amd", "host", "PoseError.hpp")).read()
    cs = open(os.path.join(ROOT, "bindings", "csharp", "HipPHDNavigator.cs")).read()
    assert "phd_pose_error(nav_" in hpp and "PoseErrorSeries PoseError(" in hpp
    assert "PoseSubtract(" in metric and "PoseAdd(" in metric and '#include "Loopy.hpp"' in metric
    assert "phd_pose_error(HandleRef nav" in cs and "DevicePoseError(" in cs
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md", os.path.join("profiles", "pose_error_cost.md")):
        assert "phd_pose_error" in open(os.path.join(ROOT, doc)).read(), doc
    assert os.path.exists(os.path.join(ROOT, "scripts", "pose_error_cost.py"))


def test_replay_refuses_pose_error_without_the_logs():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import replay
    for kw in ({"posted": False, "estimate": "waypoints"}, {"posted": True, "estimate": "poses"}, {"posted": True, "estimate": "waypoints", "pose_error": "average"}):
        kw.setdefault("pose_error", "timed")
        try:
            replay.replay({}, 4, 1, None, **kw)
        except ValueError:
            continue
        raise AssertionError("replay accepted %r" % kw)


def test_reference_entry_is_the_binary_search_of_the_plot():
    """Plot.cs:99-101 over List.BinarySearch: a hit, the first entry behind a miss, 0 behind the end"""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import replay
    times = [0.0, 0.5, 1.0, 1.5, 2.0]
    assert [replay.reference_entry(times, t) for t in (0.0, 1.0, 2.0, 0.2, 1.7, -1.0, 2.5)] == [0, 2, 4, 1, 4, 0, 0]
    assert replay.slam_time_of({"tags.out": "0.1 hello\n0.5 SLAM mode on\n0.9 SLAM mode on"}) == 0.5
    assert replay.slam_time_of({"tags.out": "0.1 SLAM mode off"}) == 0.0 and replay.slam_time_of({}) == 0.0
