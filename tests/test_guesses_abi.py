"""The boundary of phd_quasi_guesses_multi without a GPU: the entry point is declared, exported, bound and listed, its kernels
are in the gfx950 code object and use no scratch, a NULL handle is refused with the outputs untouched, the wrappers, hosts and
documents carry the members, and the two stages of loopy.GuidedFitMixtures compose to what the function gave before the split."""
import ctypes as C
import inspect
import os
import re

import numpy as np

from loopy_stub import OracleNav
from monorfs_amd import _lib, loopy
from monorfs_amd.abi import PHD_ERR_BAD_ARGUMENT, prm3d_defaults
from test_ascent_multi_abi import frames, resources_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_guess_count", "k_guess_offsets", "k_guess_emit")


def test_symbol_is_declared_exported_bound_and_listed():
    header = open(os.path.join(ROOT, "include", "phdhip.h")).read()
    lib = C.CDLL(_lib.build())
    assert "int phd_quasi_guesses_multi(phd_navigator* nav, int nproblems," in header
    assert "#define PHD_API_VERSION 4" in header              # detected by symbol: no version bump
    source = open(os.path.join(ROOT, "monorfs_amd", "csrc", "phdhip.hip")).read()
    assert hasattr(lib, "phd_quasi_guesses_multi"), "libphdhip.so does not export phd_quasi_guesses_multi"
    assert "phd_quasi_guesses_multi" in _lib.EXPORTS
    assert re.search(r"^int phd_quasi_guesses_multi\(phd_navigator\* nav, int nproblems,", source, re.M)
    bound = _lib.load().phd_quasi_guesses_multi
    # the prototype: nav, nproblems, 2 x (offsets, pool), linearpoints7, pose0s6, farpose7, radius, capacity, and six outputs
    assert bound.restype is C.c_int and len(bound.argtypes) == 17
    declared = re.search(r"int phd_quasi_guesses_multi\((.*?)\);", header, re.S).group(1)
    assert len(re.sub(r"/\*.*?\*/", "", declared, flags=re.S).split(",")) == 17
    assert bound.argtypes[9] is C.c_double and bound.argtypes[10] is C.c_int
    assert "phd_guesses.h" in _lib.SOURCES
    kernels = open(os.path.join(ROOT, "monorfs_amd", "csrc", "phd_guesses.h")).read()
    for k in KERNELS:
        assert "void %s(" % k in kernels, k
    assert kernels.count("guess_lane(g, f, q, t, tid, j, m, guess6)") == 2     # both passes through the same fit


def test_kernels_are_in_the_code_object_without_scratch():
    found = resources_of(_lib.build(), ("k_guess_",))
    assert len(found) == 3, sorted(found)
    for k in KERNELS:
        (name, (lds, scratch, vgprs)), = [(n, v) for n, v in found.items() if k in n]
        print("%-16s LDS %5d scratch %4d VGPRs %3d" % (k, lds, scratch, vgprs))
        assert scratch == 0, (k, scratch)


def test_null_handle_is_refused_with_the_outputs_untouched():
    lib = _lib.load()
    d = lambda a: a.ctypes.data_as(_lib.dp)
    i = lambda a: a.ctypes.data_as(_lib.ip)
    off = np.zeros(2, np.int32)
    lin, pose0, far = np.array([[0, 0, 0, 1.0, 0, 0, 0]]), np.zeros((1, 6)), np.array([1e5, 1e5, 1e5, 1.0, 0, 0, 0])
    goff, pairs = np.full(2, 7, np.int32), np.full((4, 2), 7, np.int32)
    g6, p7, values, empty = np.full((4, 6), 7.0), np.full((4, 7), 7.0), np.full(4, 7.0), np.full(1, 7.0)
    rc = lib.phd_quasi_guesses_multi(None, 1, i(off), None, i(off), None, d(lin), d(pose0), d(far), 0.5, 4, i(goff), i(pairs), d(g6), d(p7), d(values), d(empty))
    assert rc == PHD_ERR_BAD_ARGUMENT
    assert all(np.all(a == 7) for a in (goff, pairs, g6, p7, values, empty))


def test_wrappers_hosts_and_documents_have_the_members():
    from monorfs_amd import navigator
    sig = inspect.signature(navigator.PHDNavigator.QuasiGuessesMulti)
    assert list(sig.parameters) == ["self", "problems", "pose0s", "radius"] and sig.parameters["radius"].default == 0.5
    sig = inspect.signature(loopy.GuidedFitMixturesRouted)
    assert list(sig.parameters)[-1] == "device_guesses" and sig.parameters["device_guesses"].default is False
    sig = inspect.signature(loopy.MapMessageMixturesRouted)
    assert list(sig.parameters)[-1] == "device_guesses" and sig.parameters["device_guesses"].default is False
    for name in ("HostGuesses", "DeviceGuesses", "FitMixturesFromGuesses"):
        assert hasattr(loopy, name), name
    hpp = open(os.path.join(ROOT, "monorfs_amd", "host", "PHDNavigator.hpp")).read()
    mirror = open(os.path.join(ROOT, "monorfs_amd", "host", "Loopy.hpp")).read()
    cs = open(os.path.join(ROOT, "bindings", "csharp", "HipPHDNavigator.cs")).read()
    assert "phd_quasi_guesses_multi(nav_" in hpp and "GuessesResult QuasiGuessesMulti(" in hpp
    assert "bool device_guesses = false" in mirror and "nav.QuasiGuessesMulti(" in mirror
    assert "phd_quasi_guesses_multi(HandleRef nav" in cs and "DeviceGuidedGuesses(" in cs
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md", os.path.join("profiles", "guesses_cost.md")):
        assert "phd_quasi_guesses_multi" in open(os.path.join(ROOT, doc)).read(), doc
    assert "Pose-search guesses" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert os.path.exists(os.path.join(ROOT, "scripts", "guesses_cost.py"))
    assert os.path.exists(os.path.join(ROOT, "tests", "guesses_check.cpp"))


class BatchNav(OracleNav):
    """the oracle stub with the three multi calls of the host pipeline, each the list of its per-problem single calls"""

    def QuasiSetLogLikelihoodMulti(self, problems, poses, problem):
        return np.array([self.QuasiSetLogLikelihood(problems[q][1], problems[q][0], [p])[0] for p, q in zip(np.asarray(poses).reshape(-1, 7), problem)])

    def QuasiSetLogLikelihoodGradientMulti(self, problems, poses, problem, average_mode=0):
        r = [self.QuasiSetLogLikelihoodGradient(problems[q][1], problems[q][0], [p], average_mode) for p, q in zip(np.asarray(poses).reshape(-1, 7), problem)]
        return np.array([v[0] for v, _ in r]), np.array([g[0] for _, g in r])

    def QuasiAscentMulti(self, problems, initial, problem, average_mode=0, max_iterations=1000):
        out = [loopy.LogLikeGradientAscent(self, s, problems[q][1], problems[q][0], problems[q][2], average_mode, max_iterations=max_iterations)
               for s, q in zip(np.asarray(initial).reshape(-1, 6), problem)]
        return np.array([p for p, _ in out]), np.array([v for _, v in out]), None, False


def test_the_two_stages_compose_to_the_per_frame_fits():
    """HostGuesses then FitMixturesFromGuesses, on a stub whose multi calls are lists of single calls, is frame by frame
    GuidedFitMixture: the split moved code, it did not change what the host route computes"""
    params = prm3d_defaults(max_particles=256, max_components=600, max_measurements=16)
    pose0s, zs, models, lins = frames(params)
    stub = BatchNav(params)
    got = loopy.GuidedFitMixtures(stub, pose0s, zs, models, lins, 1, max_iterations=3)
    problems, starts = loopy._problems_of(pose0s, zs, models, lins)
    guesses, firsts, empties, pairs = loopy.HostGuesses(stub, problems, starts)
    assert [p[0] for p in pairs] == [(-1, -1)] * 3 and all(len(g) == len(f) == len(p) for g, f, p in zip(guesses, firsts, pairs))
    assert all(np.array_equal(g[0], s) for g, s in zip(guesses, starts))
    assert len(guesses[2]) == 1                               # no measurements: pose0 alone
    for i in range(3):
        want = loopy.GuidedFitMixture(OracleNav(params), pose0s[i], zs[i], models[i], lins[i], 1, max_iterations=3)
        assert got[i][0] == want[0] == empties[i] and len(got[i][1]) == len(want[1])
        for (w, m, c), (ww, wm, wc) in zip(got[i][1], want[1]):
            assert w == ww and np.array_equal(m, wm) and np.array_equal(c, wc)
    assert len(got[0][1]) >= 1
