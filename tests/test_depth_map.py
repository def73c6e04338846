"""The Kinect model's depth map without a GPU: the ABI surface (header, EXPORTS, the built library), kinect_defaults against
the reference's constants, and the numpy reading of KinectMeasurer.FuzzyVisibleM (tests/kinect_ref.py) on hand-worked
cases and against the PRM3D second reading; the CPU oracle's reading of the same rule (orc.set_depth_map) against the numpy
one, bit for bit, and whole oracle stages with a map against the numpy second readings with the Kinect PD put in."""
import ctypes
import os
import re

import numpy as np
import pytest

import kinect_ref
import orc
import test_oracle_crosscheck as second
from monorfs_amd import _lib
from monorfs_amd.abi import PHD_MODEL_PRM3D, kinect_defaults, prm3d_defaults
from monorfs_amd.synth import Frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["phd_set_depth_map", "phd_test_detection_probability"]


def test_the_two_calls_are_declared_listed_and_exported():
    header = open(os.path.join(ROOT, "include", "phdhip.h")).read()
    assert re.search(r"int\s+phd_set_depth_map\s*\(\s*phd_navigator\s*\*\s*nav\s*,\s*const\s+float\s*\*\s*depth\s*,\s*int\s+width\s*,\s*int\s+height\s*\)", header)
    assert re.search(r"int\s+phd_test_detection_probability\s*\(\s*phd_navigator\s*\*\s*nav\s*,\s*const\s+double\s*\*\s*z3\s*,\s*int\s+n\s*,\s*double\s*\*\s*out\s*\)", header)
    assert "#define PHD_DEPTH_MAX 4096" in header
    for name in NEW:
        assert name in _lib.EXPORTS
    if not os.path.exists(_lib.SO_PATH):
        pytest.skip("libphdhip.so is not built")
    lib = ctypes.CDLL(_lib.SO_PATH)
    for name in NEW:
        getattr(lib, name)


@pytest.mark.parametrize("delta,film", [(1, (-293, -213, 586, 426)), (2, (-133, -93, 266, 186)), (4, (-53, -33, 106, 66))])
def test_kinect_defaults_are_the_track_vehicles_measurer(delta, film):
    p, res = kinect_defaults(8, 300, 40, delta=delta)
    assert res == (640 // delta, 480 // delta)
    assert p.model == PHD_MODEL_PRM3D
    assert p.measurer[0] == 575.8156 / delta
    assert p.measurer[1] == float(np.float32(0.1)) and p.measurer[2] == float(np.float32(4.0))
    assert tuple(p.measurer[3:7]) == film
    assert (p.max_particles, p.max_components, p.max_measurements) == (8, 300, 40)
    d = prm3d_defaults(8, 300, 40)
    for f in ("R", "visibility_ramp", "birth_covariance"):
        assert list(getattr(p, f)) == list(getattr(d, f))
    for f in ("pd", "clutter_density", "birth_weight", "min_weight", "max_quantity", "gate_metric", "merge_threshold"):
        assert getattr(p, f) == getattr(d, f)


def _kp():
    p, (resx, resy) = kinect_defaults(1, 64, 8, delta=4)   # film x in [-53, 53], y in [-33, 33], image 160 x 120
    return p, resx, resy


def test_pixel_truncation_at_cell_edges():
    p, w, h = _kp()
    depth = np.full((h, w), np.inf, np.float32)
    depth[:, 85] = 0.5                                       # column 85 occludes (X in [5, 6) after the + 80)
    depth[45, :] = 0.5                                       # row 45 occludes (Y in [-15, -14))
    z = np.array([[4.999999, 0, 1.0], [5.0, 0, 1.0], [5.999999, 0, 1.0], [6.0, 0, 1.0],
                  [0, -15.0, 1.0], [0, -14.000001, 1.0], [0, -14.0, 1.0], [0, -15.000001, 1.0]])
    pd = kinect_ref.detection_probability(p, z, depth)
    full = kinect_ref.detection_probability(p, z, None)
    assert np.all(full == p.pd)
    assert list(pd == 0) == [False, True, True, False, True, True, False, False]
    x, y, inside = kinect_ref.pixel(depth, z)
    assert list(x[:4]) == [84, 85, 85, 86] and list(y[4:]) == [45, 45, 46, 44] and inside.all()


def test_truncation_toward_zero_and_outside_the_image():
    p = prm3d_defaults(1, 64, 8)                             # film (-320, -240, 640, 480): pixels beyond a small map
    depth = np.full((120, 160), np.inf, np.float32)
    depth[0, 0] = 0.5
    z = np.array([[-80.5, -60.5, 1.0],                       # xd = -0.5 -> (int) 0: pixel (0, 0), occluded
                  [-81.0, 0, 1.0],                           # xd = -1: outside
                  [80.0, 0, 1.0], [79.99, 0, 1.0],           # xd = 160: outside; 159.99: the last column
                  [0, 60.0, 1.0], [0, -61.0, 1.0]])
    pd = kinect_ref.detection_probability(p, z, depth)
    assert list(pd) == [0.0, 0.0, 0.0, p.pd, 0.0, 0.0]


def test_depth_in_front_behind_inside_the_ramp_and_holes():
    p, w, h = _kp()
    ramp2 = p.visibility_ramp[2]
    r = 1.0
    z = np.array([[0, 0, r]] * 6)
    cases = [r + 1.0, r - 0.5, r + 0.3 * ramp2, np.nan, 0.05, r]   # in front, behind, in the ramp, no reading, below RangeClip.Min, at the range
    out = []
    for dv in cases:
        depth = np.full((h, w), np.inf, np.float32)
        depth[60, 80] = dv
        out.append(kinect_ref.detection_probability(p, z[:1], depth)[0])
    f32 = np.float32
    assert out[0] == p.pd
    assert out[1] == 0.0
    assert out[2] == float(f32(r + 0.3 * ramp2) - f32(r)) / ramp2 * p.pd and 0.25 * p.pd < out[2] < 0.35 * p.pd
    assert out[3] == 0.0
    assert out[4] == 0.0
    assert out[5] == 0.0


def test_the_float32_range_term():
    p, w, h = _kp()
    ramp2 = p.visibility_ramp[2]
    depth = np.full((h, w), np.inf, np.float32)
    for r in (0.1 + 0.25 * ramp2, 0.1 + 0.5 * ramp2, 0.1 + 0.999 * ramp2, 0.1000001):
        got = kinect_ref.detection_probability(p, np.array([[0, 0, r]]), depth)[0]
        t32 = float(np.float32(r) - np.float32(0.1)) / ramp2
        t64 = (r - float(np.float32(0.1))) / ramp2
        assert got == max(0.0, min(1.0, t32, t64)) * p.pd
    # below RangeClip.Min: base is 0 whatever the map says
    assert kinect_ref.detection_probability(p, np.array([[0, 0, 0.09]]), depth)[0] == 0.0


def test_an_all_inf_map_is_the_prm3d_value_bit_for_bit():
    """With nothing occluding, the Kinect value is the PRM3D one, bit for bit — except inside the near range ramp
    [RangeClip.Min, RangeClip.Min + ramp[2]), where KinectMeasurer's float32 range term (KinectMeasurer.cs:169) can be the
    smaller of the two by a float32 rounding (the reference's own arithmetic: kept, include/phdhip.h)."""
    rng = np.random.default_rng(7)
    p = prm3d_defaults(1, 64, 8)
    n = 100000
    z = np.column_stack([rng.uniform(-330, 330, n), rng.uniform(-250, 250, n), rng.uniform(0.0, 2.1, n)])
    depth = np.full((480, 640), np.inf, np.float32)
    got = kinect_ref.detection_probability(p, z, depth)
    want = np.array([second.detection_probability_m(p, zz) for zz in z])
    assert np.array_equal(kinect_ref.detection_probability(p, z, None), want)
    near = (z[:, 2] >= float(np.float32(0.1))) & (z[:, 2] < float(np.float32(0.1)) + p.visibility_ramp[2])
    assert np.array_equal(got[~near], want[~near])
    assert np.all(got[near] <= want[near]) and np.allclose(got[near], want[near], rtol=0, atol=1e-6)
    assert np.count_nonzero(got[near] != want[near]) > 0   # (the float32 term does bind there)


# ---- the oracle's reading of the same rule (orc_set_depth_map; oracle/phd_oracle.cpp kinect_visible) ----------------------

def _oracle_points(rng, p, w, h, n):
    """probe points (cell edges and one ulp either side) and a few ranges that are +inf or overflow float32: there base is
    0 and the depth term inf - inf is NaN, which only the `base == 0` early return turns into 0"""
    z = kinect_ref.probe_points(rng, w, h, n)
    k = n // 50
    z[-k:, 2] = np.where(rng.uniform(size=k) < 0.5, np.inf, 1e39)
    return z


@pytest.mark.parametrize("which", ["prm3d_640x480", "kinect_160x120"])
def test_oracle_detection_probability_is_the_numpy_reading_bit_for_bit(which):
    rng = np.random.default_rng(111 if which.startswith("prm3d") else 112)
    if which.startswith("prm3d"):
        p, (w, h) = prm3d_defaults(1, 600, 8), (640, 480)
        p.measurer[2] = float(np.float32(4.0))
    else:
        p, (w, h) = kinect_defaults(1, 600, 8, delta=4)
    z = _oracle_points(rng, p, w, h, 200000)
    with np.errstate(invalid="ignore", over="ignore"):
        assert np.array_equal(orc.detection_probability_m(p, z), kinect_ref.detection_probability(p, z, None))   # no map
        depth = kinect_ref.probe_map(rng, w, h)
        depth[rng.uniform(size=depth.shape) < 0.1] = np.inf   # (the +inf pixels the +inf ranges land on)
        with orc.depth_map(depth):
            got = orc.detection_probability_m(p, z)
        want = kinect_ref.detection_probability(p, z, depth)
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, "%d of %d differ, first %r: %r vs %r" % (len(bad), len(z), z[bad[0]], got[bad[0]], want[bad[0]])
        near = (z[:, 2] >= float(np.float32(0.1))) & (z[:, 2] < float(np.float32(0.1)) + p.visibility_ramp[2])
        assert np.count_nonzero((want > 0) & (want < p.pd) & ~near) > 100   # the occlusion ramp
        assert np.count_nonzero((want > 0) & (want < p.pd) & near) > 100    # the float32 range term
        assert np.count_nonzero(want == 0) > 1000 and np.count_nonzero(want == p.pd) > 1000
        # a map smaller than the film: points whose pixel is outside it give 0
        small = np.full((h // 4, w // 4), np.inf, np.float32)
        small[::3, ::2] = 0.7
        with orc.depth_map(small):
            got = orc.detection_probability_m(p, z)
        _, _, inside = kinect_ref.pixel(small, z)
        assert np.all(got[~inside] == 0) and np.count_nonzero(~inside) > 1000
        assert np.array_equal(got, kinect_ref.detection_probability(p, z, small))
    # the context manager leaves no map behind
    assert np.array_equal(orc.detection_probability_m(p, z[:1000]), kinect_ref.detection_probability(p, z[:1000], None))


def test_oracle_pixel_truncation_and_the_row_major_layout():
    """hand-worked pixels on a non-square 160 x 120 map: (int) truncates toward zero, x picks the column, y the row"""
    p, w, h = _kp()
    depth = np.full((h, w), np.inf, np.float32)
    depth[:, 85] = 0.5
    depth[45, :] = 0.5
    depth[0, 0] = np.nan
    z = np.array([[4.999999, 0, 1.0], [5.0, 0, 1.0], [5.999999, 0, 1.0], [6.0, 0, 1.0],
                  [0, -15.0, 1.0], [0, -14.000001, 1.0], [0, -14.0, 1.0], [0, -15.000001, 1.0],
                  [-80.5, -60.5, 1.0], [-53.0, -33.0, 1.0], [-53.0 + 1e-9, -33.0 + 1e-9, 1.0]])
    with orc.depth_map(depth):
        got = orc.detection_probability_m(p, z)
    want = kinect_ref.detection_probability(p, z, depth)
    assert np.array_equal(got, want)
    assert list(got[:8] == 0) == [False, True, True, False, True, True, False, False]
    assert got[8] == 0.0     # outside the film (base 0) on the NaN pixel
    assert got[9] == 0.0     # on the film's corner: base is 0
    assert 0 < got[10] < 1e-9   # just inside it: the PRM3D ramp, the map's +inf pixel does not bind


def test_oracle_and_the_device_layout_agree_on_a_transposed_map():
    """a map whose transpose is a different frame: reading depth[x][y] (the reference's jagged array) instead of the
    library's depth[y][x] would give other values"""
    p, w, h = _kp()
    rng = np.random.default_rng(3)
    depth = kinect_ref.occluding_map(rng, w, h, near=0.5, far=1.5, blocks=(16, 12), holes=0.05)
    z = np.column_stack([rng.uniform(-53, 53, 5000), rng.uniform(-33, 33, 5000), rng.uniform(0.3, 1.8, 5000)])
    with orc.depth_map(depth):
        got = orc.detection_probability_m(p, z)
    assert np.array_equal(got, kinect_ref.detection_probability(p, z, depth))
    assert np.count_nonzero(got != kinect_ref.detection_probability(p, z, None)) > 1000


def _landmark_map(p, pose, lm, depths, w=640, h=480):
    """an all-+inf 640 x 480 map with a 9 x 9 block of depth depths[j] (a callable of the range, or a value) around each
    landmark's pixel"""
    d = np.full((h, w), np.inf, np.float32)
    for m, dv in zip(lm, depths):
        zh = second.measure_perfect(p, pose, m)
        x, y = int(zh[0] + w / 2), int(zh[1] + h / 2)
        d[max(0, y - 4):y + 5, max(0, x - 4):x + 5] = dv(zh[2]) if callable(dv) else dv
    return d


def _kinect_pd(depth):
    return lambda pp, z: float(kinect_ref.detection_probability(pp, z, depth)[0])


@pytest.mark.parametrize("seed", range(6))
def test_oracle_correct_with_kinect_pd_against_numpy(seed, monkeypatch):
    """CorrectConditional with the Kinect PD: the oracle against the numpy second reading with kinect_ref's PD put in
    (as tests/test_gpu_depth_map.py does for the device). Each case has an occluded landmark (PD 0), one inside the depth
    ramp (0 < PD < p.pd), and one without a reading or seen in full."""
    rng = np.random.default_rng(1400 + seed)
    p = prm3d_defaults(4, 600, 8)
    pose, lm, z = second.random_case(rng, p, 4, 5)
    pred = second.random_mixture(rng, lm, 0.3, 1.1)
    ramp2 = p.visibility_ramp[2]
    depth = _landmark_map(p, pose, lm, [lambda r: r - 0.3, lambda r: r + 0.45 * ramp2, np.nan if seed % 2 else np.inf,
                                        lambda r: r + 0.05 * ramp2])
    pd = kinect_ref.detection_probability(p, np.array([second.measure_perfect(p, pose, m) for m in pred[1]]), depth)
    assert pd[0] == 0 and 0 < pd[1] < p.pd and 0 < pd[3] < p.pd
    monkeypatch.setattr(second, "detection_probability_m", _kinect_pd(depth))
    comps = second.numpy_correct(p, pose, z, pred, by_value=False)
    with orc.depth_map(depth):
        ow, om, oc = orc.correct(p, pose, z, pred)
        pw, pm, pc = orc.predict(p, pose, z, pred)
    assert len(ow) == len(comps)
    for i, (w, m, P) in enumerate(comps):
        assert np.isclose(ow[i], w, rtol=1e-9, atol=1e-300), (i, ow[i], w)
        assert np.allclose(om[i], m, rtol=1e-9, atol=1e-12)
        assert np.allclose(oc[i], P, rtol=1e-8, atol=1e-14)
    # the map does not touch the prediction (PD enters the correction only)
    qw, qm, qc = orc.predict(p, pose, z, pred)
    assert np.array_equal(pw, qw) and np.array_equal(pm, qm) and np.array_equal(pc, qc)


@pytest.mark.parametrize("seed", range(10))
def test_oracle_set_log_likelihood_with_kinect_pd_against_all_permutations(seed, monkeypatch):
    """SetLogLikeMatrix's pdj with the Kinect PD (log PD and log(1 - PD) of PD = 0, of a ramp value and of p.pd) against
    the brute force over all permutations of tests/test_oracle_crosscheck.py, with kinect_ref's PD put in"""
    rng = np.random.default_rng(1500 + seed)
    p = prm3d_defaults(4, 600, 8)
    J = int(rng.integers(1, 4))
    M = int(rng.integers(1, 6 - J))
    pose, lm, z = second.random_case(rng, p, J, M)
    ramp2 = p.visibility_ramp[2]
    kinds = [lambda r: r - 0.3, lambda r: r + 0.45 * ramp2, np.nan, np.inf, lambda r: r + 0.8 * ramp2]
    depth = _landmark_map(p, pose, lm, [kinds[(seed + j) % len(kinds)] for j in range(J)])
    monkeypatch.setattr(second, "detection_probability_m", _kinect_pd(depth))
    with np.errstate(divide="ignore"):
        want = second.set_log_likelihood_bruteforce(p, pose, lm, z)
    with orc.depth_map(depth):
        got = orc.set_log_likelihood(p, pose, lm, z)[0]
        quasi = orc.quasi_set_log_likelihood(p, pose, lm, z)
    assert np.isclose(got, want, rtol=1e-10, atol=1e-10), (got, want)
    assert quasi == orc.quasi_set_log_likelihood(p, pose, lm, z)   # the quasi set log-likelihood keeps the constant PD


def test_oracle_all_inf_map_is_no_map_bit_for_bit():
    """An all-+inf map changes nothing when no measurement lies in the near range ramp: whole oracle steps (predict,
    correct, prune, set log-likelihood, alpha, resampling) over two frames, bit for bit"""
    f = Frame(24, 64, 16, 1601, weight_profile="steady")
    f.z[:, 2] = np.maximum(f.z[:, 2], 0.25)
    p = prm3d_defaults(max_particles=f.P, max_components=600, max_measurements=f.M)
    runs = []
    for depth in (None, np.full((480, 640), np.inf, np.float32)):
        st = orc.State(f.P, 600)
        st.poses[:] = f.poses
        st.w[:, :f.C], st.mean[:, :f.C], st.cov[:, :f.C], st.n[:] = f.w, f.mean, f.cov, f.C
        out = []
        with orc.depth_map(depth):
            for step, u in enumerate((0.31, 0.77)):
                best, src, res, alpha = orc.slam_update(p, st, f.z + 0.3 * step, u=u, threads=4)
                out.append((best, src, res, alpha, st.copy()))
        runs.append(out)
    for (b0, s0, r0, a0, t0), (b1, s1, r1, a1, t1) in zip(*runs):
        assert b0 == b1 and r0 == r1 and np.array_equal(s0, s1) and np.array_equal(a0, a1)
        assert np.array_equal(t0.weights, t1.weights) and np.array_equal(t0.n, t1.n)
        for k in ("w", "mean", "cov"):
            assert np.array_equal(getattr(t0, k), getattr(t1, k))


def test_oracle_occluding_map_changes_the_step():
    """and a real occluding map does change it (the map reaches slam_update's parallel region)"""
    f = Frame(8, 64, 16, 1602, weight_profile="steady")
    f.z[:, 2] = np.maximum(f.z[:, 2], 0.25)
    p = prm3d_defaults(max_particles=f.P, max_components=600, max_measurements=f.M)
    alphas = []
    for depth in (None, kinect_ref.occluding_map(np.random.default_rng(4), 640, 480)):
        st = orc.State(f.P, 600)
        st.poses[:] = f.poses
        st.w[:, :f.C], st.mean[:, :f.C], st.cov[:, :f.C], st.n[:] = f.w, f.mean, f.cov, f.C
        with orc.depth_map(depth):
            alphas.append(orc.slam_update(p, st, f.z, u=0.5, threads=4)[3])
    assert np.all(alphas[0] != alphas[1])
