"""The boundary of phd_map_error without a GPU: the entry point is declared, exported and bound, refuses a NULL handle with its
outputs untouched, and the wrapper, the hosts, the replay script and the record reader carry the new members."""
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
    assert "int phd_map_error(phd_navigator* nav, const double* truth3, int ntruth, double cutoff, double order," in header
    assert hasattr(lib, "phd_map_error"), "libphdhip.so does not export phd_map_error"
    assert "phd_map_error" in _lib.EXPORTS
    assert "phd_maperror.h" in _lib.SOURCES
    bound = _lib.load().phd_map_error
    assert bound.restype is C.c_int and len(bound.argtypes) == 13
    assert "#define PHD_API_VERSION 4" in header              # detected by symbol: no version bump
    # the bound the header states is the one the kernel is built for
    kernel = open(os.path.join(ROOT, "monorfs_amd", "csrc", "phd_maperror.h")).read()
    stated = int(re.search(r"#define PHD_MAP_ERROR_MAX (\d+)", header).group(1))
    assert stated == int(re.search(r"#define PHD_MAPERR_MAX (\d+)", kernel).group(1)) and stated >= 257


def test_null_handle_is_refused():
    lib = _lib.load()
    n = C.c_int(0)
    t, o, c, s, z = _lib.dp(), _lib.dp(), _lib.dp(), _lib.dp(), _lib.ip()
    truth = np.zeros(3)
    rc = lib.phd_map_error(None, truth.ctypes.data_as(_lib.dp), 1, 1.0, 1.0, None, None, C.byref(n), C.byref(t), C.byref(o), C.byref(c), C.byref(s), C.byref(z))
    assert rc == PHD_ERR_BAD_ARGUMENT
    assert n.value == 0 and not any((t, o, c, s, z))


def test_wrapper_hosts_and_scripts_have_the_members():
    from monorfs_amd import navigator
    from monorfs_amd import recordio as rio
    sig = inspect.signature(navigator.PHDNavigator.MapError)
    assert list(sig.parameters)[:5] == ["self", "truth", "cutoff", "order", "align"]
    assert sig.parameters["cutoff"].default == 1.0 and sig.parameters["order"].default == 1.0 and sig.parameters["align"].default is None
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import replay
    assert inspect.signature(replay.replay).parameters["map_error"].default is False
    assert "vismaps.out" in rio.OPTIONAL_MEMBERS and "vismaps.out" not in rio.MEMBERS
    hpp = open(os.path.join(ROOT, "monorfs_amd", "host", "PHDNavigator.hpp")).read()
    cs = open(os.path.join(ROOT, "bindings", "csharp", "HipPHDNavigator.cs")).read()
    assert "phd_map_error(nav_" in hpp and "MapErrorEntry" in hpp
    assert "phd_map_error(HandleRef nav" in cs and "MapError(List<double[]> truth" in cs
    for doc in ("INTEGRATION.md", "README.md"):
        assert "phd_map_error" in open(os.path.join(ROOT, doc)).read(), doc


def test_visited_map_keeps_each_seen_landmark_once():
    """the rule of Ospa.hpp::VisitedMap in scripts/replay.py: weight > 0, and nothing kept within 1e-5"""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import replay
    a, b, c = [0.5, 0.25, 1.2], [-0.3, 0.1, 0.9], [0.05, -0.4, 1.5]
    frames = [(np.array([1.0, 0.0]), np.array([a, b])),                       # b is visible but not measured
              (np.array([1.0, 1.0, 1.0]), np.array([a, np.add(a, [3e-6, 0, 0]), c])),
              (np.array([1.0]), np.array([b]))]
    got = replay.visited_map(frames)
    assert got.shape == (3, 3) and np.array_equal(got, np.array([a, c, b]))
    assert replay.visited_map([]).shape == (0, 3)
    rec = {"scene.world": open(os.path.join(ROOT, "tests", "golden", "record", "scene.world")).read()}
    assert np.array_equal(replay.truth_of(rec), np.array([a, b, c]))
    from monorfs_amd import recordio as rio
    rec["vismaps.out"] = rio.serialize_maps([(0.0, (frames[0][0], frames[0][1], np.tile(np.eye(3), (2, 1, 1))))])
    assert np.array_equal(replay.truth_of(rec), np.array([a]))
