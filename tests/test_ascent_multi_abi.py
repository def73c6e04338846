"""The boundary of phd_quasi_ascent_multi / phd_quasi_set_loglik_multi without a GPU: the entry points are declared, exported and
bound, a NULL handle is refused with the outputs untouched, the wrappers, hosts and documents carry the members,
loopy.GuidedFitMixtures on a stub without the multi calls is the list of the per-frame fits, and the rebinding wrappers of
phd_ascent_multi.h use no more scratch and the same LDS as the evaluation kernels of phd_ascent.h."""
import ctypes as C
import inspect
import os
import re
import struct
import subprocess
import tempfile

import numpy as np

from loopy_stub import OracleNav, scene
from monorfs_amd import _lib, loopy
from monorfs_amd.abi import PHD_ERR_BAD_ARGUMENT, prm3d_defaults
from monorfs_amd.navigator import pose3d_add

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (seed, landmarks, measurements, the small vector that makes the scene's own linearisation pose)
FRAMES = [(91, 6, 5, [0.02, -0.01, 0.015, 0.03, -0.02, 0.01]), (92, 3, 2, [-0.01, 0.02, 0.0, -0.015, 0.025, 0.02]), (93, 4, 0, [0.0, 0.01, -0.02, 0.01, 0.01, -0.03])]


def frames(params):
    """(pose0s, measurement sets, models, linearisation poses) of the three scenes"""
    pose0s, zs, models, lins = [], [], [], []
    for seed, J, M, shift in FRAMES:
        rng = np.random.default_rng(seed)
        lin, lm, z = scene(rng, params, J, M, sigma=0.3)
        pose0s.append(rng.normal(0, 1, 6) * [4e-3, 4e-3, 4e-3, 2e-3, 2e-3, 2e-3])
        zs.append(z)
        models.append((np.full(len(lm), 1.0001), lm, np.broadcast_to(1e-4 * np.eye(3), (len(lm), 3, 3))))
        lins.append(pose3d_add(lin, shift))
    return pose0s, zs, models, lins


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "phdhip.h")).read()
    lib = C.CDLL(_lib.build())
    assert "int phd_quasi_ascent_multi(phd_navigator* nav, int nproblems," in header
    assert "int phd_quasi_set_loglik_multi(phd_navigator* nav, int nproblems," in header
    assert "#define PHD_API_VERSION 4" in header              # detected by symbol: no version bump
    source = open(os.path.join(ROOT, "monorfs_amd", "csrc", "phdhip.hip")).read()
    for name, nargs in (("phd_quasi_ascent_multi", 17), ("phd_quasi_set_loglik_multi", 12)):
        assert hasattr(lib, name), "libphdhip.so does not export %s" % name
        assert name in _lib.EXPORTS
        assert re.search(r"^int %s\(phd_navigator\* nav, int nproblems," % name, source, re.M), name
        bound = getattr(_lib.load(), name)
        assert bound.restype is C.c_int and len(bound.argtypes) == nargs
    assert "phd_ascent_multi.h" in _lib.SOURCES
    kernels = open(os.path.join(ROOT, "monorfs_amd", "csrc", "phd_ascent_multi.h")).read()
    for k in ("k_multi_setll", "k_multi_setll_grad"):
        assert "void %s(" % k in kernels, k
    assert "struct QuasiProblems" in kernels
    single = open(os.path.join(ROOT, "monorfs_amd", "csrc", "phd_ascent.h")).read()
    assert "const int* problem;" in single and "void k_ascent_setll(" in single and "void k_ascent_setll_grad(" in single


def test_null_handle_is_refused_with_the_outputs_untouched():
    lib = _lib.load()
    d = lambda a: a.ctypes.data_as(_lib.dp)
    i = lambda a: a.ctypes.data_as(_lib.ip)
    off, which = np.zeros(2, np.int32), np.zeros(2, np.int32)
    start, lin = np.zeros((2, 6)), np.array([[0, 0, 0, 1.0, 0, 0, 0]])
    poses, values, iters, hess = np.full((2, 6), 7.0), np.full(2, 7.0), np.full(2, 7, np.int32), np.full((2, 6, 6), 7.0)
    rc = lib.phd_quasi_ascent_multi(None, 1, i(off), None, i(off), None, d(lin), d(start), i(which), 2, 0, 10, 0, d(poses), d(values), i(iters), d(hess))
    assert rc == PHD_ERR_BAD_ARGUMENT
    assert np.all(poses == 7) and np.all(values == 7) and np.all(iters == 7) and np.all(hess == 7)
    out, grad = np.full(2, 7.0), np.full((2, 6), 7.0)
    rc = lib.phd_quasi_set_loglik_multi(None, 1, i(off), None, i(off), None, d(np.tile(lin, (2, 1))), i(which), 2, 0, d(out), d(grad))
    assert rc == PHD_ERR_BAD_ARGUMENT
    assert np.all(out == 7) and np.all(grad == 7)


def test_wrappers_hosts_and_documents_have_the_members():
    from monorfs_amd import navigator
    sig = inspect.signature(navigator.PHDNavigator.QuasiAscentMulti)
    assert list(sig.parameters) == ["self", "problems", "initial", "problem", "average_mode", "max_iterations", "round_iterations", "hessians"]
    assert sig.parameters["max_iterations"].default == 1000 and sig.parameters["round_iterations"].default == 0 and sig.parameters["hessians"].default is False
    assert list(inspect.signature(navigator.PHDNavigator.QuasiSetLogLikelihoodMulti).parameters) == ["self", "problems", "poses", "problem"]
    assert list(inspect.signature(navigator.PHDNavigator.QuasiSetLogLikelihoodGradientMulti).parameters) == ["self", "problems", "poses", "problem", "average_mode"]
    assert list(inspect.signature(loopy.GuidedFitMixtures).parameters) == ["nav", "pose0s", "measurement_sets", "models", "linearpoints", "average_mode", "max_iterations"]
    assert list(inspect.signature(loopy.MapMessageMixtures).parameters) == ["nav", "trajectory", "factors", "pose0s", "linearpoints", "to", "average_mode"]
    hpp = open(os.path.join(ROOT, "monorfs_amd", "host", "PHDNavigator.hpp")).read()
    mirror = open(os.path.join(ROOT, "monorfs_amd", "host", "Loopy.hpp")).read()
    cs = open(os.path.join(ROOT, "bindings", "csharp", "HipPHDNavigator.cs")).read()
    assert "phd_quasi_ascent_multi(nav_" in hpp and "AscentResult QuasiAscentMulti(" in hpp and "phd_quasi_set_loglik_multi(nav_" in hpp
    assert "QuasiSetLogLikelihoodMulti(" in hpp and "QuasiSetLogLikelihoodGradientMulti(" in hpp
    assert "GuidedFitMixtures(" in mirror and "MapMessageMixtures(" in mirror and "nav.QuasiAscentMulti(" in mirror
    assert "phd_quasi_ascent_multi(HandleRef nav" in cs and "phd_quasi_set_loglik_multi(HandleRef nav" in cs and "DeviceLogLikeGradientAscentMulti(" in cs
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md", os.path.join("profiles", "ascent_multi_cost.md")):
        assert "phd_quasi_ascent_multi" in open(os.path.join(ROOT, doc)).read(), doc
    assert "Pose searches of many frames" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert os.path.exists(os.path.join(ROOT, "scripts", "ascent_multi_cost.py"))
    assert os.path.exists(os.path.join(ROOT, "tests", "ascent_multi_check.cpp"))


def test_fallback_is_the_list_of_the_per_frame_fits():
    params = prm3d_defaults(max_particles=256, max_components=600, max_measurements=16)
    pose0s, zs, models, lins = frames(params)
    assert [(len(m[1]), len(z)) for m, z in zip(models, zs)] == [(6, 5), (3, 2), (4, 0)]
    assert len({tuple(l) for l in lins}) == 3
    stub = OracleNav(params)
    assert not hasattr(stub, "QuasiAscentMulti")
    got = loopy.GuidedFitMixtures(stub, pose0s, zs, models, lins, 1)
    want = [loopy.GuidedFitMixture(OracleNav(params), pose0s[i], zs[i], models[i], lins[i], 1) for i in range(3)]
    assert len(got) == 3
    for (empty, comps), (wempty, wcomps) in zip(got, want):
        assert empty == wempty and len(comps) == len(wcomps)
        for (w, m, c), (ww, wm, wc) in zip(comps, wcomps):
            assert w == ww and np.array_equal(m, wm) and np.array_equal(c, wc)
    assert len(got[0][1]) >= 1                                  # a frame with measurements does fit a component
    # No measurements: pose0 is the only guess and the set likelihood is flat — the far pose's value exactly —, so GuidedFitMixture
    # does not drop it (:821-823 drops a guess that is WORSE), the climb gains nothing and the one component it leaves has no
    # weight and no covariance. (The reference never fits such a frame, :527-530: MapMessageMixtures gives it (0.0, []).)
    first = stub.QuasiSetLogLikelihood(zs[2], loopy.best_map_estimate(models[2]), [pose3d_add(lins[2], pose0s[2])])
    assert got[2][0] == first[0] and len(got[2][1]) == 1
    weight, mean, cov = got[2][1][0]
    assert weight == 0 and np.array_equal(mean, pose0s[2]) and not np.any(cov)


def resources_of(so, wanted):
    """{kernel: (static LDS bytes, private segment bytes, VGPRs)} of the gfx950 kernels whose names contain one of `wanted`, from
    the code object's metadata (as tests/test_abi_exports.py::static_lds_of reads the LDS)"""
    blob = open(so, "rb").read()
    at = blob.find(b"__CLANG_OFFLOAD_BUNDLE__")
    assert at >= 0, "no offload bundle in %s" % so
    count, = struct.unpack_from("<Q", blob, at + 24)
    pos, image = at + 32, None
    for _ in range(count):
        off, size, tlen = struct.unpack_from("<QQQ", blob, pos)
        triple = blob[pos + 24:pos + 24 + tlen]
        pos += 24 + tlen
        if b"gfx950" in triple:
            image = blob[at + off:at + off + size]
    assert image, "no gfx950 code object in %s" % so
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(image)
        f.flush()
        readelf = os.path.join(os.path.dirname(os.path.dirname(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))), "llvm", "bin", "llvm-readelf")
        notes = subprocess.check_output([readelf, "--notes", f.name]).decode()
    found = {}
    for block in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:   # (the first key of every kernel's record)
        name = re.search(r"\.name:\s*(\S+)", block).group(1)
        if any(k in name for k in wanted):
            field = lambda key: int(re.search(r"\.%s:\s*(\d+)" % key, block).group(1))
            found[name] = (field("group_segment_fixed_size"), field("private_segment_fixed_size"), field("vgpr_count"))
    return found


def test_rebinding_wrappers_cost_no_scratch_and_no_lds():
    """a wrapper that rebinds four fields of the argument block must not spill it: per ZB the private segment of k_multi_setll
    [_grad] is at most that of k_ascent_setll[_grad], the static LDS the same (a condition; the VGPR counts are printed)"""
    found = resources_of(_lib.build(), ("k_multi_setll", "k_ascent_setll"))
    assert len(found) == 12, sorted(found)
    for zb in (1, 2, 4):
        for base, multi in (("k_ascent_setll", "k_multi_setll"), ("k_ascent_setll_grad", "k_multi_setll_grad")):
            pick = lambda stem: [v for k, v in found.items() if re.search(r"\d%sILi%dE" % (stem, zb), k)]
            (a,), (m,) = pick(base), pick(multi)
            print("ZB %d %-20s LDS %6d scratch %5d VGPRs %3d | %-20s LDS %6d scratch %5d VGPRs %3d" % ((zb, base) + a + (multi,) + m))
            assert m[1] <= a[1], (zb, multi, m, a)
            assert m[0] == a[0], (zb, multi, m, a)
