"""The boundary of phd_step_hold_async without a GPU: the entry point is declared, exported and bound, the kernels' file is a
source of the library, the API version has not moved, a NULL handle is refused, and the wrapper, the hosts and the documents
carry the new members."""
import ctypes as C
import inspect
import os

from monorfs_amd import _lib
from monorfs_amd.abi import PHD_ERR_BAD_ARGUMENT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "phdhip.h")).read()
    lib = C.CDLL(_lib.build())
    assert "int phd_step_hold_async(phd_navigator* nav, int held);" in header
    assert hasattr(lib, "phd_step_hold_async"), "libphdhip.so does not export phd_step_hold_async"
    assert "phd_step_hold_async" in _lib.EXPORTS
    assert "phd_hold.h" in _lib.SOURCES and os.path.exists(os.path.join(_lib.CSRC, "phd_hold.h"))
    bound = _lib.load().phd_step_hold_async
    assert bound.restype is C.c_int and list(bound.argtypes) == [C.c_void_p, C.c_int]
    assert "#define PHD_API_VERSION 4" in header              # detected by symbol: no version bump
    assert _lib.load().phd_api_version() == 4
    kernels = open(os.path.join(_lib.CSRC, "phd_hold.h")).read()
    assert "k_hold_save" in kernels and "k_hold_restore" in kernels


def test_null_handle_is_refused():
    lib = _lib.load()
    for held in (-1, 0, 3):
        assert lib.phd_step_hold_async(None, held) == PHD_ERR_BAD_ARGUMENT


def test_wrapper_hosts_and_documents_have_the_members():
    from monorfs_amd import loopy, navigator
    assert list(inspect.signature(navigator.PHDNavigator.StepHold).parameters) == ["self", "held"]
    sig = inspect.signature(loopy.LeaveOneOutMaps)
    assert list(sig.parameters) == ["nav", "trajectory", "factors", "indices", "to"]
    assert sig.parameters["indices"].default is None and sig.parameters["to"].default is None
    nav_hpp = open(os.path.join(ROOT, "monorfs_amd", "host", "PHDNavigator.hpp")).read()
    loopy_hpp = open(os.path.join(ROOT, "monorfs_amd", "host", "Loopy.hpp")).read()
    cs = open(os.path.join(ROOT, "bindings", "csharp", "HipPHDNavigator.cs")).read()
    assert "void StepHold(int held)" in nav_hpp and "phd_step_hold_async(nav_, held)" in nav_hpp
    assert "inline std::vector<Map> LeaveOneOutMaps(" in loopy_hpp and "StepHold(" in loopy_hpp
    assert "int    phd_step_hold_async(HandleRef nav, int held);" in cs and "DeviceLeaveOneOutMaps(" in cs
    for doc in ("INTEGRATION.md", "README.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "phd_step_hold_async" in text and "LeaveOneOutMaps" in text, doc
    assert "## Leave-one-out maps" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
