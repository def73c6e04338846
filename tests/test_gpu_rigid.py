"""The pose-dependent device code at real rotations. monorfs_amd/synth.py keeps every particle pose next to the identity
(quaternion imaginary parts of 2.5e-4) and every component fully visible, so a transposed off-diagonal pair of R(q*), a
sign on one product of quaternion parts or a wrong branch behind the camera would pass the other modules. Here every
frame is a synthetic one with components planted in the six visibility ramp bands, out of view and behind the camera
(rigid.plant_edges), moved as a whole by a rigid motion (rigid.transport; the poses of rigid.POSES: quarter turns about
each axis, qw = 0, the axis permutation, a generic one with qw < 0, one that is not normalised).

Every input comes from the table in tests/rigid.py; tests/test_oracle_rigid.py shows on the host, against the oracle
alone, that each of them bites, sits on no discrete edge, and that the oracle itself agrees with the numpy second
reading at these poses and is invariant under the transport. Helpers and tolerances are those of
tests/test_gpu_shape_edges.py (stages, the path step after each case) and tests/oracle_parity.py (whole steps)."""
import numpy as np
import pytest

import orc
import rigid
from oracle_parity import assert_step_matches, oracle_state
from test_gpu_shape_edges import (THREADS, assert_path, biting_map, klass, launches, make, path_of, stage_parity, upload,
                                  whole_steps)

pytestmark = pytest.mark.gpu


def assert_zero_pd_copies(nav, p, f, want, depth):
    """every planted component of detection probability 0 (out of the film, beyond a range clip, behind the camera; behind
    the depth map where there is one): the device's corrected list holds its misdetection copy with the prior weight,
    bit for bit, and nothing else of it — the oracle's detection updates from it weigh exactly 0, and the device's list,
    as long as the oracle's above MinWeight (stage_parity), holds nothing below MinWeight"""
    for i in range(f.P):
        with orc.depth_map(depth):
            zero = rigid.zero_pd_planted(p, f, i)
        assert len(zero) >= 5
        pred, cor = want[i][0], want[i][1]
        src, det = rigid.correct_sources(p, f.poses[i], f.z, pred)
        assert len(src) == len(cor[0])
        gw, gm, _ = nav.CorrectConditional(i)
        assert np.all(gw >= p.min_weight), "particle %d: a corrected component below MinWeight" % i
        for j in zero:
            assert np.any(det & (src == j)) and np.all(cor[0][det & (src == j)] == 0)
            hit = np.nonzero((gm == f.mean[i, j]).all(axis=1))[0]
            assert len(hit) == 1, "particle %d: %d corrected components at the mean of planted component %d" % (i, len(hit), j)
            assert gw[hit[0]] == f.w[i, j], "particle %d planted %d: the copy weighs %r, the prior %r" % (i, j, gw[hit[0]], f.w[i, j])


@pytest.mark.parametrize("case", list(rigid.STAGE_CASES))
def test_stages_at_a_pose(monkeypatch, case):
    """every stage of every particle against the oracle, the PD = 0 copies, then the path step"""
    pose, C, M, env, timed, depth = rigid.STAGE_CASES[case]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    f = rigid.stage_frame(case)
    nav, p = make(f)
    if timed:
        nav.set_frozen(True)
        nav.set_all_pairs(True)
    d = biting_map(p, oracle_state(f, p.max_quantity), f.z, rigid.stage_seed(case), case) if depth else None
    want = stage_parity(nav, p, f, f.z, d)
    assert_zero_pd_copies(nav, p, f, want, d)
    assert_path(nav, [(f.z, d)], launches(path_of(f.P, M, env)), case)
    nav.close()


@pytest.mark.parametrize("case", list(rigid.STEP_CASES))
def test_whole_steps_at_a_pose(monkeypatch, case):
    """three SlamUpdates from a transported planted frame, every particle after every step; `unnorm` is not here: a whole
    step compares the stored poses exactly, and the oracle stores what it is handed"""
    pose, P, M, env = rigid.STEP_CASES[case]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    f = rigid.step_frame(case)
    nav, p = make(f)
    whole_steps(nav, p, f, rigid.step_seed(case), False, False, case)
    assert_path(nav, [(f.z, None)], launches(path_of(P, M, env)), case)
    nav.close()


def test_turning_trajectory():
    """six steps of 0.55 rad yaw and 0.05 m forward from y90 (qw goes from 0.7 through 0 to -0.7): the motion step on
    the device against orc.update_motion, then (the oracle goes on from the device's poses, as in
    test_gpu_round4.test_perfect_particle_wins_most_often) a whole step on what particle 0 sees of the frame's landmarks"""
    f = rigid.turn_frame()
    nav, p = make(f, max_measurements=rigid.TURN_MAX_M)
    st = oracle_state(f, p.max_quantity)
    landmarks = rigid.turning_landmarks(f)
    qw = [f.poses[0, 3]]
    for s, step in enumerate(rigid.turning_plan(f, rigid.TURN_SEED)):
        what = "%s step %d" % (rigid.TURN_CASE, s)
        nav.UpdateOdometry(None, rigid.TURN_READING, step["noise"])
        poses = nav.poses()
        assert np.allclose(poses, orc.update_motion(st.poses, rigid.TURN_READING, step["noise"]), rtol=0, atol=1e-14), what + ": the motion step"
        st.poses[:] = poses
        z = rigid.turning_measurements(p, poses[0], landmarks, step)
        best, src, res, _ = orc.slam_update(p, st, z, u=step["u"], threads=THREADS)
        nav.SlamUpdate(None, z, u_resample=step["u"])
        assert_step_matches(nav, st, best, src, res, p.max_quantity, what)
        qw.append(st.poses[0, 3])
    assert qw[0] > 0.3 and qw[-1] < -0.3
    assert_path(nav, [(z, None)], launches("chain"), rigid.TURN_CASE)
    nav.close()


# ---- the device against itself: a frame and the same frame moved ------------------------------------------------------
INVARIANCE = {"%s-M%d-%s-%s" % (pose, M, klass(M), path_of(4, M, env)): (pose, M, env)
              for M, env in ((32, rigid.CHAIN), (64, rigid.SEPARATE)) for pose in rigid.INVARIANCE_POSES}


def device_stages(nav, f):
    nav.run_stages(f.z, with_alpha=True)
    alpha, setll = nav.WeightAlpha(), nav.SetLogLikelihood()
    return [(nav.PredictConditional(i), nav.CorrectConditional(i), nav.PruneModel(i), alpha[i], setll[i]) for i in range(f.P)]


@pytest.mark.parametrize("case", list(INVARIANCE))
def test_device_is_invariant_under_rigid_transport(monkeypatch, case):
    """no oracle: the device's stages on the planted frame moved by a pose, mapped back, against its stages on the frame
    as it is — the checks and tolerances of test_oracle_rigid.test_oracle_is_invariant_under_rigid_transport (the corrected
    mixture as a set: the device emits it in no fixed order)"""
    pose, M, env = INVARIANCE[case]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    seed = rigid.FRAME_SEEDS[4, 120, M]
    f0 = rigid.planted(4, 120, M, seed)
    nav, p = make(f0)
    base = device_stages(nav, f0)
    assert all(np.isfinite(b[3]) and b[3] > 0 and np.isfinite(b[4]) for b in base)
    f = rigid.transport(f0, rigid.POSES[pose])
    upload(nav, f)
    moved = device_stages(nav, f)
    for i in range(f.P):
        rigid.assert_invariant(base[i], moved[i], rigid.POSES[pose], "%s particle %d" % (case, i), corrected_in_order=False)
    assert_path(nav, [(f.z, None)], launches(path_of(4, M, env)), case)
    nav.close()


# ---- the quasi set log-likelihood and its gradient --------------------------------------------------------------------
@pytest.mark.parametrize("case", list(rigid.QUASI_CASES))
def test_quasi_set_log_likelihood_and_gradient_at_a_pose(case):
    """the batch of test_gpu_parity.test_quasi_set_log_likelihood_batch / _gradient_batch (48 candidate poses around the
    camera, measurements crowding one landmark) with the landmarks and the poses moved by the case's pose: the value
    kernel, and value and gradient in both readings of TemperedAverage, with their tolerances. (The kernel timers do not
    cover the quasi kernels: these ids name the landmark arrays' place, LDS or the HBM slab, by the rule of
    test_gpu_shape_edges, and no path step follows.)"""
    from test_gpu_parity import make_nav, quasi_maxq
    from monorfs_amd import navigator
    f, lm, z, poses = rigid.quasi_batch(case)
    nav, p = make_nav(navigator, f, maxq=quasi_maxq(len(lm)))
    got = nav.QuasiSetLogLikelihood(z, lm, poses)
    want = np.array([orc.quasi_set_log_likelihood(p, poses[i], lm, z) for i in range(f.P)])
    assert np.all(np.isfinite(want))
    assert np.allclose(got, want, rtol=1e-9, atol=1e-9), np.max(np.abs(got - want))
    for mode in (0, 1):
        got, ggot = nav.QuasiSetLogLikelihoodGradient(z, lm, poses, average_mode=mode)
        ref = [orc.quasi_set_log_likelihood_grad(p, poses[i], lm, z, mode) for i in range(f.P)]
        wv, wg = np.array([r[0] for r in ref]), np.array([r[1] for r in ref])
        assert np.allclose(got, wv, rtol=1e-9, atol=1e-9), (mode, np.max(np.abs(got - wv)))
        assert np.allclose(ggot, wg, rtol=1e-8, atol=1e-7), (mode, np.max(np.abs(ggot - wg)))
        assert np.max(np.abs(wg)) > 1
    nav.close()
