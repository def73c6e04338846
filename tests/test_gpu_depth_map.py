"""The Kinect model's depth map on the device (phd_set_depth_map, phd_test_detection_probability): the probe against the
numpy reading of KinectMeasurer.FuzzyVisibleM (tests/kinect_ref.py), whole steps where the map reduces to something known
(all +inf: no map; all NaN: pd = 0), an occluding map at stage level against the numpy second readings with the Kinect PD
put in, stream order, the multi-device handle, clearing, bad arguments, and the quasi set log-likelihood it must not touch."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import kinect_ref
import orc
import test_oracle_crosscheck as second
from monorfs_amd.abi import PHD_ERR_BAD_ARGUMENT, PHD_MODEL_LINEAR2D, kinect_defaults, params_from_dict, prm3d_defaults
from monorfs_amd.synth import CONFIGS, Frame

pytestmark = pytest.mark.gpu

W, H = 640, 480   # the default PRM3D film is the whole 640 x 480 image


@pytest.fixture(scope="module")
def nav_mod():
    from monorfs_amd import navigator
    return navigator


def frame(cfg):
    P, C_, M, seed = CONFIGS[cfg]
    f = Frame(P, C_, M, seed, weight_profile="steady")
    # (measurements — and so births and updates — out of the near range ramp [0.1, 0.195): there KinectMeasurer's float32 range
    # term can round below the PRM3D double one, and an all-+inf map would not be the PRM3D path bit for bit; tests/test_depth_map.py)
    f.z[:, 2] = np.maximum(f.z[:, 2], 0.25)
    return f


def make(nav_mod, f, timed=False, devices=None, **over):
    p = prm3d_defaults(max_particles=f.P, max_components=600, max_measurements=max(f.M, 1))
    for k, v in over.items():
        setattr(p, k, v)
    nav = nav_mod.PHDNavigator(p, particlecount=f.P, devices=devices)
    nav.upload_state(f.planes(), f.counts, f.poses, f.weights)
    if timed:
        nav.set_frozen(True)
        nav.set_all_pairs(True)
    return nav, p


def snapshot(nav):
    src, res = nav.resample_sources()
    maps = [nav.MapModel(i) for i in range(nav.particle_count)]
    return nav.VehicleWeights, src, res, nav.BestParticle, maps


def assert_same(a, b, what):
    wa, sa, ra, ba, ma = a
    wb, sb, rb, bb, mb = b
    assert np.array_equal(wa, wb), "%s: weights differ" % what
    assert ra == rb and np.array_equal(sa, sb), "%s: resample sources differ" % what
    assert ba == bb, "%s: best particle differs" % what
    for i, (x, y) in enumerate(zip(ma, mb)):
        for u, v in zip(x, y):
            assert u.shape == v.shape and np.array_equal(u, v), "%s: map of particle %d differs" % (what, i)


def run_steps(nav, f, nsteps=3):
    out = []
    for s in range(nsteps):
        nav.SlamUpdate(None, f.z, u_resample=0.25 + 0.2 * s)
        out.append(snapshot(nav))
    return out


def occluder(seed, w=W, h=H):
    return kinect_ref.occluding_map(np.random.default_rng(seed), w, h, near=0.5, far=1.5, blocks=(8, 6), holes=0.05)


# ---- 1. the probe -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["prm3d_640x480", "kinect_160x120"])
def test_probe_is_the_numpy_reading_bit_for_bit(nav_mod, which):
    rng = np.random.default_rng(11 if which.startswith("prm3d") else 12)
    if which.startswith("prm3d"):
        p, (w, h) = prm3d_defaults(1, 600, 8), (W, H)
        p.measurer[2] = float(np.float32(4.0))
    else:
        p, (w, h) = kinect_defaults(1, 600, 8, delta=4)
    nav = nav_mod.PHDNavigator(p, particlecount=1)
    z = kinect_ref.probe_points(rng, w, h, 500000)
    assert np.array_equal(nav.DetectionProbabilityM(z), kinect_ref.detection_probability(p, z, None))   # no map: PRM3D
    depth = kinect_ref.probe_map(rng, w, h)
    nav.set_depth_map(depth)
    got = nav.DetectionProbabilityM(z)
    want = kinect_ref.detection_probability(p, z, depth)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, "%d of %d differ, first %r: %r vs %r" % (len(bad), len(z), z[bad[0]], got[bad[0]], want[bad[0]])
    assert 0 < np.count_nonzero((want > 0) & (want < p.pd)) and np.count_nonzero(want == p.pd) > 0
    # a smaller map than the film: points whose pixel is outside it give 0
    small = np.full((h // 4, w // 4), np.inf, np.float32)
    nav.set_depth_map(small)
    _, _, inside = kinect_ref.pixel(small, z)
    got = nav.DetectionProbabilityM(z)
    assert np.all(got[~inside] == 0) and np.count_nonzero(~inside) > 1000
    assert np.array_equal(got, kinect_ref.detection_probability(p, z, small))
    nav.close()


# ---- 2. / 3. maps that reduce to known paths ---------------------------------------------------------------------
PATHS = [("A24", False), ("A", False), ("B1024", False), ("A24", True), ("A", True), ("B1024", True)]


@pytest.mark.parametrize("cfg,timed", PATHS)
def test_all_inf_map_is_no_map(nav_mod, cfg, timed):
    f = frame(cfg)
    a, _ = make(nav_mod, f, timed)
    b, _ = make(nav_mod, f, timed)
    b.set_depth_map(np.full((H, W), np.inf, np.float32))
    for s, (x, y) in enumerate(zip(run_steps(a, f), run_steps(b, f))):
        assert_same(x, y, "%s step %d" % (cfg, s))
    a.close(), b.close()


@pytest.mark.parametrize("cfg,timed", PATHS)
def test_all_nan_map_is_pd_zero(nav_mod, cfg, timed):
    f = frame(cfg)
    a, _ = make(nav_mod, f, timed, pd=0.0)
    b, _ = make(nav_mod, f, timed)
    b.set_depth_map(np.full((H, W), np.nan, np.float32))
    for s, (x, y) in enumerate(zip(run_steps(a, f), run_steps(b, f))):
        assert_same(x, y, "%s step %d" % (cfg, s))
    a.close(), b.close()


def test_all_nan_map_against_the_oracle_with_pd_zero(nav_mod):
    f = frame("A")
    nav, p = make(nav_mod, f)
    nav.set_depth_map(np.full((H, W), np.nan, np.float32))
    p.pd = 0.0
    st = orc.State(f.P, 700)
    st.poses[:] = f.poses
    st.w[:, :f.C], st.mean[:, :f.C], st.cov[:, :f.C], st.n[:] = f.w, f.mean, f.cov, f.C
    best, src, res, _ = orc.slam_update(p, st, f.z, u=0.37, threads=8)
    nav.SlamUpdate(None, f.z, u_resample=0.37)
    gsrc, gres = nav.resample_sources()
    assert gres == res and np.array_equal(gsrc, src) and nav.BestParticle == best
    assert np.allclose(nav.VehicleWeights, st.weights, rtol=1e-6, atol=1e-300)
    iu = np.triu_indices(3)
    for i in range(f.P):
        w, m, c = nav.MapModel(i)
        ow, om, oc = st.map(i)
        assert len(w) == len(ow)
        assert np.allclose(w, ow, rtol=1e-7) and np.allclose(m, om, rtol=1e-7, atol=1e-11)
        assert np.allclose(c[:, iu[0], iu[1]], oc[:, iu[0], iu[1]], rtol=1e-7, atol=1e-13)
    nav.close()


# ---- 4. an occluding map at stage level --------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["A", "B512"])
def test_misdetection_copies_are_one_minus_kinect_pd(nav_mod, cfg):
    f = frame(cfg)
    nav, p = make(nav_mod, f)
    depth = occluder(21)
    nav.set_depth_map(depth)
    nav.run_stages(f.z, with_alpha=True)
    moved = total = 0
    for i in range(f.P):
        pw, pm, _ = nav.PredictConditional(i)
        zh = np.array([orc.measure_perfect(p, f.poses[i], m) for m in pm])
        pd = kinect_ref.detection_probability(p, zh, depth)
        pd0 = kinect_ref.detection_probability(p, zh, None)
        moved += np.count_nonzero(pd != pd0)
        total += len(pd)
        assert np.array_equal(nav.DetectionProbabilityM(zh), pd)
        cw, cm, _ = nav.CorrectConditional(i)
        have = {}
        for w, m in zip(cw, cm):
            have.setdefault(m.tobytes(), []).append(w)
        for w, m, d in zip(pw, pm, pd):
            wm = (1 - d) * w
            if wm < p.min_weight:
                continue
            assert wm in have.get(m.tobytes(), []), "particle %d: no misdetection copy of weight (1 - PD) w = %r" % (i, wm)
    assert moved >= 0.2 * total, "the map moved the PD of %d of %d components only" % (moved, total)
    nav.close()


def test_corrected_mixture_against_numpy_with_kinect_pd(nav_mod, monkeypatch):
    f = frame("A")
    nav, p = make(nav_mod, f)
    depth = occluder(22)
    nav.set_depth_map(depth)
    nav.run_stages(f.z, with_alpha=True)
    monkeypatch.setattr(second, "detection_probability_m", lambda pp, z: float(kinect_ref.detection_probability(pp, z, depth)[0]))
    iu = np.triu_indices(3)
    for i in np.random.default_rng(5).choice(f.P, 16, replace=False):
        pred = nav.PredictConditional(i)
        comps = [c for c in second.numpy_correct(p, f.poses[i], f.z, pred, by_value=False) if not c[0] < p.min_weight]
        gw, gm, gc = nav.CorrectConditional(i)
        assert len(gw) == len(comps), "particle %d: %d corrected components, numpy keeps %d" % (i, len(gw), len(comps))
        used = np.zeros(len(gw), bool)
        for w, m, P in comps:
            d = np.abs(gw - w) / abs(w) + np.max(np.abs(gm - m), axis=1) / (np.abs(m).max() + 1e-9)
            d[used] = np.inf
            j = int(np.argmin(d))
            assert np.isclose(gw[j], w, rtol=1e-9, atol=0) and np.allclose(gm[j], m, rtol=1e-9, atol=1e-12), (i, w, gw[j])
            assert np.allclose(gc[j][iu], P[iu], rtol=1e-8, atol=1e-14)
            used[j] = True
    nav.close()


@pytest.mark.parametrize("seed", range(6))
def test_set_log_likelihood_and_alpha_with_kinect_pd(nav_mod, monkeypatch, seed):
    f = Frame(4, 3, 2, 600 + seed, weight_profile="steady")
    f.z[:, 2] = np.maximum(f.z[:, 2], 0.25)
    nav, p = make(nav_mod, f)
    depth = occluder(30 + seed)
    nav.set_depth_map(depth)
    nav.run_stages(f.z, with_alpha=True)
    setll, alpha = nav.SetLogLikelihood(), nav.WeightAlpha()
    monkeypatch.setattr(second, "detection_probability_m", lambda pp, z: float(kinect_ref.detection_probability(pp, z, depth)[0]))
    checked = 0
    for i in range(f.P):
        pred, corr = nav.PredictConditional(i), nav.PruneModel(i)
        jm, _ = second.best_map_estimate(corr)
        if len(jm) + f.M > 5:
            continue
        sll = second.set_log_likelihood_bruteforce(p, f.poses[i], jm, f.z)
        plog = sum(np.log(second.mixture(x, pred)) for x in jm)
        clog = sum(np.log(second.mixture(x, corr)) for x in jm)
        want = np.exp(sll + (plog - np.sum(pred[0])) - (clog - np.sum(corr[0])))
        assert np.isclose(setll[i], sll, rtol=1e-9, atol=1e-12), (i, setll[i], sll)
        assert np.isclose(alpha[i], want, rtol=1e-9, atol=0), (i, alpha[i], want)
        checked += 1
    assert checked > 0
    nav.close()


# ---- 5. stream order ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["A", "B1024"])
def test_maps_posted_between_steps_keep_stream_order(nav_mod, cfg):
    f = frame(cfg)
    maps = [occluder(40 + s) for s in range(3)]
    us = [0.3, 0.5, 0.7]
    runs = []
    for mode in ("posted", "synced", "blocking"):
        nav, _ = make(nav_mod, f)
        for s in range(3):
            nav.set_depth_map(maps[s])
            if mode == "blocking":
                nav.SlamUpdate(None, f.z, u_resample=us[s])
            else:
                nav.set_measurements(f.z)
                nav.step_async(us[s])
                if mode == "synced":
                    nav.sync()
        nav.sync()
        runs.append(snapshot(nav))
        nav.close()
    assert_same(runs[0], runs[1], "posted vs synced")
    assert_same(runs[0], runs[2], "posted vs blocking")


# ---- 6. / 7. the multi-device handle, clearing the map -----------------------------------------------------------
def test_multi_device_handle_with_a_map(nav_mod):
    f = frame("A")
    depth = occluder(50)
    a, _ = make(nav_mod, f)
    b, _ = make(nav_mod, f, devices=[0, 0])
    a.set_depth_map(depth)
    b.set_depth_map(depth)
    for s, (x, y) in enumerate(zip(run_steps(a, f), run_steps(b, f))):
        assert_same(x, y, "multi step %d" % s)
    a.close(), b.close()


def test_clearing_the_map_is_the_prm3d_path(nav_mod):
    f = frame("A")
    a, _ = make(nav_mod, f)
    a.set_depth_map(occluder(60))
    run_steps(a, f, 2)
    planes, counts, poses, weights = a.download_state(600)
    a.set_depth_map(None)
    b, _ = make(nav_mod, f)
    b.upload_state(planes, counts, poses, weights)
    for s, (x, y) in enumerate(zip(run_steps(a, f), run_steps(b, f))):
        assert_same(x, y, "cleared step %d" % s)
    a.close(), b.close()


# ---- 8. bad arguments ----------------------------------------------------------------------------------------------
def test_bad_arguments_leave_the_map_and_the_state(nav_mod):
    f = frame("A")
    depth = occluder(70)
    a, _ = make(nav_mod, f)
    b, _ = make(nav_mod, f)
    a.set_depth_map(depth)
    b.set_depth_map(depth)
    lib, h = a._lib, a._h
    buf = np.zeros(16, np.float32)
    fp = buf.ctypes.data_as(C.POINTER(C.c_float))
    for args in [(fp, 0, 4), (fp, 4, 0), (fp, 4097, 1), (fp, 1, 4097), (fp, -1, 4), (None, 4, 4), (None, 0, 4), (None, 640, 480)]:
        assert lib.phd_set_depth_map(h, *args) == PHD_ERR_BAD_ARGUMENT, args
    for s, (x, y) in enumerate(zip(run_steps(a, f, 1), run_steps(b, f, 1))):
        assert_same(x, y, "after the refused calls")
    a.close(), b.close()
    kat = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "phdnavigator_kat.json")))
    p = params_from_dict(kat["params"], max_particles=4, max_components=600, max_measurements=8)
    assert p.model == PHD_MODEL_LINEAR2D
    lin = nav_mod.PHDNavigator(p, particlecount=4, pose=(0, 0, 0, 1, 0, 0, 0))
    assert lin._lib.phd_set_depth_map(lin._h, fp, 4, 4) == PHD_ERR_BAD_ARGUMENT
    assert lin._lib.phd_set_depth_map(lin._h, None, 0, 0) == PHD_ERR_BAD_ARGUMENT
    lin.close()


# ---- 9. the quasi set log-likelihood keeps the constant PD ----------------------------------------------------------
def test_quasi_set_log_likelihood_ignores_the_map(nav_mod):
    rng = np.random.default_rng(80)
    p = prm3d_defaults(64, 600, 64)
    nav = nav_mod.PHDNavigator(p, particlecount=64)
    pose, lm, z = second.random_case(rng, p, 24, 40)
    poses = np.array([np.concatenate([pose[:3] + rng.normal(0, 0.01, 3), pose[3:]]) for _ in range(32)])
    v0 = nav.QuasiSetLogLikelihood(z, lm, poses)
    g0 = nav.QuasiSetLogLikelihoodGradient(z, lm, poses)
    nav.set_depth_map(occluder(81))
    v1 = nav.QuasiSetLogLikelihood(z, lm, poses)
    g1 = nav.QuasiSetLogLikelihoodGradient(z, lm, poses)
    assert np.array_equal(v0, v1) and np.array_equal(g0[0], g1[0]) and np.array_equal(g0[1], g1[1])
    nav.close()
