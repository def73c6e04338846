"""The device away from prm3d_defaults: the stages of a step, whole steps, the pose searches, the Kinect branch, the
Linear2D model and the logs at the named parameter sets of tests/paramspace.py, against the CPU oracle (tests/orc.py) with
the tolerances of tests/test_gpu_parity.py (stages) and tests/oracle_parity.py (whole steps).

Every frame is made for its parameter block (paramspace.frame_for) and meets its preconditions on the oracle before the
device is asked anything; tests/test_oracle_param_space.py asserts the same preconditions without a GPU."""
import json
import os

import numpy as np
import pytest

import kinect_ref
import orc
import paramspace as ps
from loopy_stub import OracleNav, scene
from monorfs_amd import loopy
from oracle_parity import assert_step_matches, oracle_state
from test_gpu_depth_oracle import assert_the_map_bites
from test_gpu_kat import KAT, z3
from test_gpu_map_history import assert_same_maps, state_entry
from test_gpu_parity import assert_mix_close, match_unordered
from test_gpu_shape_edges import THREADS, stage_parity, upload
from test_oracle_crosscheck import measure_perfect, measure_to_map

pytestmark = pytest.mark.gpu

# how a handle runs the stages: the one-launch chain (the default at these sizes), the separate kernels on two streams, and
# the mode bench.py times
MODES = {"chain": ({}, False), "separate": ({"PHD_CHAIN_MAX": "0", "PHD_SPLIT": "2"}, False), "timed": ({}, True)}


def handle(p, f, monkeypatch=None, mode="chain", devices=None):
    from monorfs_amd import navigator
    env, timed = MODES[mode]
    for k, v in env.items():
        monkeypatch.setenv(k, v)   # (read when the handle is made)
    nav = navigator.PHDNavigator(p, particlecount=f.P, devices=devices)
    upload(nav, f)
    if timed:
        nav.set_frozen(True)
        nav.set_all_pairs(True)
    return nav


# ---- stages -----------------------------------------------------------------------------------------------------------
_stage = {}


def stage_case(name, shape):
    """(params, frame) of a stage case, its preconditions asserted once"""
    if (name, shape) not in _stage:
        _stage[name, shape] = ps.checked_frame(name, *shape, ps.stage_seed(name, shape))[:2]
    return _stage[name, shape]


STAGE_IDS = [(name, shape) for name in ps.PRM3D_SETS for shape in ps.STAGE_SHAPES[name]]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name,shape", STAGE_IDS, ids=["%s-P%d-C%d-M%d" % ((n,) + s) for n, s in STAGE_IDS])
def test_stages_against_the_oracle(monkeypatch, name, shape, mode):
    """predict 1e-9, the corrected set unordered 1e-9, pruned 1e-7, set log-likelihood 1e-9, alpha 1e-6, every particle"""
    p, f = stage_case(name, shape)
    nav = handle(p, f, monkeypatch, mode)
    stage_parity(nav, p, f, f.z)
    nav.close()


def test_stages_at_detection_probability_one():
    """PD = 1: the maps against the oracle as everywhere; for the set log-likelihood and alpha every particle must be in the
    oracle's class — finite and within tolerance where the oracle is finite, -inf and 0.0 where the oracle says so; never
    NaN, never the other class"""
    p, f, want = ps.pd_one_case()
    nav = handle(p, f)
    nav.run_stages(f.z, with_alpha=True)
    alpha, setll = nav.WeightAlpha(), nav.SetLogLikelihood()
    for i, (pred, cor, pr, a, sll) in enumerate(want):
        assert_mix_close(nav.PredictConditional(i), pred, 1e-9, "predict[%d]" % i)
        keep = ~(cor[0] < p.min_weight)
        match_unordered(nav.CorrectConditional(i), tuple(x[keep] for x in cor), 1e-9)
        assert_mix_close(nav.PruneModel(i), pr, 1e-7, "prune[%d]" % i)
        assert not np.isnan(setll[i]) and not np.isnan(alpha[i]), "particle %d: NaN (%r, %r)" % (i, setll[i], alpha[i])
        if np.isfinite(sll):
            assert np.isclose(setll[i], sll, rtol=1e-9, atol=1e-9), "set log-likelihood[%d]: %r vs %r" % (i, setll[i], sll)
            assert np.isclose(alpha[i], a, rtol=1e-6, atol=0), "alpha[%d]: %r vs %r" % (i, alpha[i], a)
        else:
            assert sll == -np.inf and a == 0.0
            assert setll[i] == -np.inf and alpha[i] == 0.0, "particle %d: (%r, %r), the oracle's (-inf, 0)" % (i, setll[i], alpha[i])
    nav.close()


# ---- whole steps ------------------------------------------------------------------------------------------------------
_steps = {}


def step_case(name, shape):
    """(params, frame, the oracle's run) of a whole-step case, computed once: paramspace.oracle_steps"""
    if (name, shape) not in _steps:
        p, f, seed = ps.step_frame(name, shape)
        _steps[name, shape] = (p, f, ps.oracle_steps(name, p, f, seed, threads=THREADS))
    return _steps[name, shape]


def drive(nav, run, posted, what, stride, each=None):
    """three steps with the host moving the poses between them; posted: back to back, one sync, the final state compared"""
    for s, (poses, z, u, st, best, src, res) in enumerate(run):
        if posted:
            nav.set_poses(poses)
            nav.set_measurements(z)
            nav.step_async(u_resample=u)
        else:
            nav.Update(float(s), poses)
            nav.SlamUpdate(float(s), z, u_resample=u)
            assert_step_matches(nav, st, best, src, res, stride, "%s step %d" % (what, s))
            if each:
                each(s)
    if posted:
        nav.sync()
        assert_step_matches(nav, st, best, src, res, stride, "%s after %d posted steps" % (what, len(run)))


STEP_IDS = [(name, shape) for name in ps.STEP_SETS for shape in ps.STEP_SHAPES]


@pytest.mark.parametrize("posted", [False, True], ids=["synchronous", "posted"])
@pytest.mark.parametrize("name,shape", STEP_IDS, ids=["%s-P%d-C%d-M%d" % ((n,) + s) for n, s in STEP_IDS])
def test_whole_steps_against_the_oracle(name, shape, posted):
    p, f, run = step_case(name, shape)
    if p.min_effective_particle == 0.6:
        res = [r[6] for r in run]
        assert True in res and False in res, "resampling decisions %r" % (res,)
    nav = handle(p, f)
    drive(nav, run, posted, name, max(p.max_quantity, f.C))
    nav.close()


def test_two_shards_take_the_parameters_bit_for_bit():
    """all_of_it on a two-shard handle (the same device twice; the parameters reach every shard by a copy of their own):
    every step against the oracle, and the final state bit-equal to the single handle's"""
    name, shape = "all_of_it", ps.STEP_SHAPES[0]
    p, f, run = step_case(name, shape)
    stride = max(p.max_quantity, f.C)
    states = []
    for devices in (None, [0, 0]):
        nav = handle(p, f, devices=devices)
        drive(nav, run, False, "%s on %s" % (name, devices or "one handle"), stride)
        states.append(nav.download_state(stride) + (nav.resample_sources()[0], nav.BestParticle))
        nav.close()
    for a, b in zip(*states):
        assert np.array_equal(a, b), "the two-shard handle's state differs from the single handle's"


def test_logs_record_what_the_getters_gave():
    """all_of_it with the trajectory and the map log on: WayMaps equals what the getters gave behind each step, the paths
    hold the poses the host set"""
    name, shape = "all_of_it", ps.STEP_SHAPES[0]
    p, f, run = step_case(name, shape)
    nav = handle(p, f)
    nav.enable_history(len(run))
    nav.enable_map_history(len(run), len(run) * 600)
    want = []
    drive(nav, run, False, name + " logged", max(p.max_quantity, f.C), each=lambda s: want.append(state_entry(nav, float(s))))
    assert_same_maps(nav.WayMaps(), want, "WayMaps against the getters")
    assert all(1 <= len(e[3][0]) <= p.max_quantity for e in want)
    t, x, slots = nav.WayPoints(range(f.P))
    assert np.array_equal(t, np.arange(len(run), dtype=float))
    assert np.array_equal(x[:, -1], run[-1][0][slots[:, -1]])   # (the newest entry: the poses set before the last step, by ancestor)
    nav.close()


# ---- the pose searches ------------------------------------------------------------------------------------------------
QUASI_SETS = ["correlated", "camera", "all_of_it"]
QUASI_SHAPES = [(3, 4), (40, 30), (12, 70)]


def quasi_case(p, J, M, seed):
    """J landmarks inside p's film and clip, M measurements (of the first landmarks + N(0, R), two more crowding the first
    one, clutter), 8 candidate poses next to the identity"""
    rng = np.random.default_rng([seed, J, M])
    c = ps.Camera(p)
    L = np.linalg.cholesky(np.array(p.R).reshape(3, 3))
    zs = np.column_stack([rng.uniform(c.left + 30, c.right - 30, J), rng.uniform(c.top + 30, c.bottom - 30, J),
                          rng.uniform(c.rmin + 0.3, c.rmax - 0.3, J)])
    lm = np.array([measure_to_map(p, ps.IDENTITY, zz) for zz in zs])
    nd = min(J, int(np.ceil(0.8 * M)))
    z = np.concatenate([zs[:nd] + rng.normal(size=(nd, 3)) @ L.T,
                        np.column_stack([rng.uniform(c.left, c.right, M - nd), rng.uniform(c.top, c.bottom, M - nd),
                                         rng.uniform(c.rmin, c.rmax, M - nd)])])
    if M > 3 and J > 3:   # measurements crowding one landmark: clusters beyond 5 rows
        z[1] = z[0] + L @ [1.5, -1.0, 0.3]
        z[2] = z[0] + L @ [-2.0, 0.5, -0.6]
    poses = np.tile(ps.IDENTITY, (8, 1))
    poses[:, :3] += rng.normal(0, 5e-3, (8, 3))
    poses[:, 3:] += rng.normal(0, 2e-3, (8, 4))
    return lm, z, poses


@pytest.mark.parametrize("J,M", QUASI_SHAPES)
@pytest.mark.parametrize("name", QUASI_SETS)
def test_quasi_set_log_likelihood_and_gradient(name, J, M):
    """phd_quasi_set_loglik and phd_quasi_set_loglik_grad (both average modes) on a batch of 8 poses: the oracle call and the
    tolerances of test_gpu_parity.test_quasi_set_log_likelihood_gradient_batch. The set bites: the oracle's values move by
    more than 1e-3 when R loses its correlations / the focal length is the default's."""
    from monorfs_amd import navigator
    p = ps.params(name, P=8, C=J, M=M)
    lm, z, poses = quasi_case(p, J, M, 600 + QUASI_SETS.index(name))
    want = {mode: [orc.quasi_set_log_likelihood_grad(p, poses[i], lm, z, mode) for i in range(8)] for mode in (0, 1)}
    wv = np.array([w[0] for w in want[0]])
    assert np.all(np.isfinite(wv))
    plain = ps.with_R(p, np.diag(np.diag(np.array(p.R).reshape(3, 3))))
    plain.measurer[0] = 575.8156
    assert np.max(np.abs(wv - [orc.quasi_set_log_likelihood(plain, poses[i], lm, z) for i in range(8)])) > 1e-3
    nav = navigator.PHDNavigator(p, particlecount=8)
    got = nav.QuasiSetLogLikelihood(z, lm, poses)
    assert np.allclose(got, wv, rtol=1e-9, atol=1e-9), np.max(np.abs(got - wv))
    for mode in (0, 1):
        gv, gg = nav.QuasiSetLogLikelihoodGradient(z, lm, poses, average_mode=mode)
        wg = np.array([w[1] for w in want[mode]])
        assert np.allclose(gv, wv, rtol=1e-9, atol=1e-9), np.max(np.abs(gv - wv))
        assert np.allclose(gg, wg, rtol=1e-8, atol=1e-7), np.max(np.abs(gg - wg))
        assert np.max(np.abs(wg)) > 1
    nav.close()


def test_gradient_ascent_with_a_correlated_R():
    """monorfs_amd/loopy.py's gradient ascent driven by the device against the same host code driven by the oracle, as
    tests/test_gpu_loopy.py, at the correlated set"""
    from monorfs_amd import navigator
    nav = navigator.PHDNavigator(ps.params("correlated", P=256, M=16), particlecount=1)
    rng = np.random.default_rng(23)
    lin, lm, z = scene(rng, nav.params, 10, 7)
    starts = rng.normal(0, 1, (6, 6)) * [4e-3, 4e-3, 4e-3, 2e-3, 2e-3, 2e-3]
    got, gotv = loopy.LogLikeGradientAscent(nav, starts, z, lm, lin, 0)
    want, wantv = loopy.LogLikeGradientAscent(OracleNav(nav.params), starts, z, lm, lin, 0)
    assert np.allclose(gotv, wantv, rtol=1e-9, atol=1e-8), np.max(np.abs(gotv - wantv))
    assert np.allclose(got, want, rtol=0, atol=1e-9), np.max(np.abs(got - want))
    assert np.any(np.abs(got - starts) > 1e-5)
    nav.close()


# ---- Kinect -----------------------------------------------------------------------------------------------------------
def test_kinect_depth_branch_with_a_full_R():
    """kinect_defaults + the correlated R and a depth map of tests/kinect_ref.py: the depth branch and a full R meet in
    comp_measure<true>"""
    from monorfs_amd import navigator
    P, C, M = 4, 130, 32
    p, (w, h) = ps.kinect_params("correlated", P, M)
    f = ps.frame_for(p, P, C, M, 700)
    ps.assert_frame_bites("correlated", p, f)
    depth = kinect_ref.occluding_map(np.random.default_rng(701), w, h, near=1.5, far=4.2, blocks=(8, 6), holes=0.05)
    assert_the_map_bites(p, oracle_state(f, 600), f.z, depth, "kinect + correlated", sample=P)
    with orc.depth_map(depth):
        stages = ps.assert_frame_margins(p, f, what="kinect + correlated")
        ps.assert_set_bites("correlated", p, f, stages)
    nav = navigator.PHDNavigator(p, particlecount=P)
    upload(nav, f)
    stage_parity(nav, p, f, f.z, depth)
    nav.close()


# ---- Linear2D ---------------------------------------------------------------------------------------------------------
def test_linear2d_step_with_a_correlated_R():
    """test_gpu_kat.test_linear2d_step_against_the_oracle's procedure with R = [[5e-4, 3e-4], [3e-4, 8e-4]] and range 4.25:
    the 2 x 2 R padded into DevParams' 3 x 3, landmarks on both sides of the range"""
    from monorfs_amd import navigator
    rng = np.random.default_rng(62)
    P, C, M = 12, 10, 5
    p = ps.linear2d_params(dict(KAT["params"], min_effective_particle=0.5), max_particles=P, max_components=600, max_measurements=8)
    lm = rng.uniform(-4, 4, (C, 2))
    assert np.any(np.linalg.norm(lm, axis=1) > 4.4) and np.count_nonzero(np.linalg.norm(lm, axis=1) < 4.0) >= M
    nav = navigator.PHDNavigator(p, particlecount=P, pose=[0, 0, 0, 1, 0, 0, 0])
    st = orc.State(P, 700)
    poses = np.zeros((P, 7))
    poses[:, 3] = 1
    poses[:, :2] = rng.normal(0, 0.02, (P, 2))
    model = (rng.uniform(0.5, 1.1, C), np.column_stack([lm, np.zeros(C)]), np.broadcast_to(np.diag([2e-3, 2e-3, 1e-2]), (C, 3, 3)).copy())
    nav.reset(poses[0], model, P)
    nav.set_poses(poses)
    st.poses[:] = poses
    for i in range(P):
        st.w[i, :C], st.mean[i, :C], st.cov[i, :C], st.n[i] = model[0], model[1], model[2], C
    near = np.nonzero(np.linalg.norm(lm, axis=1) < 4.0)[0]
    for step in range(3):
        z = lm[rng.permutation(near)[:M]] + rng.multivariate_normal([0, 0], ps.LINEAR2D_R, M)
        best, src, res, _ = orc.slam_update(p, st, z, u=0.37 + 0.1 * step, threads=2)
        nav.SlamUpdate(None, z3(z), u_resample=0.37 + 0.1 * step)
        gsrc, gres = nav.resample_sources()
        assert gres == res and np.array_equal(gsrc, src) and nav.BestParticle == best
        assert np.allclose(nav.VehicleWeights, st.weights, rtol=1e-6, atol=1e-300)
        for i in (0, P - 1):
            gw, gm, gc = nav.MapModel(i)
            ow, om, oc = st.map(i)
            assert len(gw) == len(ow) and np.allclose(gw, ow, rtol=1e-7) and np.allclose(gm, om, rtol=1e-7, atol=1e-10)
            assert np.allclose(gc[:, :2, :2], oc[:, :2, :2], rtol=1e-7, atol=1e-13)
    nav.close()
