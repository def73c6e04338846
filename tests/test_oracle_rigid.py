"""The oracle (tests/orc.py) at real rotations, on the host: its cross-checks against the numpy second reading
(tests/test_oracle_crosscheck.py) at the poses of tests/rigid.py, its invariance under the rigid transport of a whole
planted frame, and, for every frame tests/test_gpu_rigid.py hands the device (the table in tests/rigid.py), that the
planted layout bites for every particle and that no input sits on a discrete edge (rigid.assert_frame_bites,
rigid.assert_margins)."""
import numpy as np
import pytest

import orc
import rigid
import test_oracle_crosscheck as xc
from oracle_parity import oracle_state
from test_gpu_shape_edges import THREADS, biting_map

POSE_IDS = list(rigid.POSES)


@pytest.fixture
def at_pose(monkeypatch, request):
    """the cross-checks below draw their cases through xc.random_case: give it the pose of the test's id, and see
    afterwards that the test drew a case at that pose (not one next to the identity through a binding of its own)"""
    q, original, drawn = rigid.POSES[request.node.callspec.params["pose"]], xc.random_case, []

    def random_case(rng, p, J, M):
        pose, lm, z = original(rng, p, J, M, pose=q)
        drawn.append(pose[3:].copy())
        return pose, lm, z

    monkeypatch.setattr(xc, "random_case", random_case)
    yield
    assert drawn and all(np.array_equal(d, q) for d in drawn), "the cross-check drew no case at the pose of its id"


@pytest.mark.parametrize("seed", range(12))
@pytest.mark.parametrize("pose", POSE_IDS)
def test_set_log_likelihood_against_all_permutations(at_pose, pose, seed):
    xc.test_set_log_likelihood_against_all_permutations(seed)


@pytest.mark.parametrize("seed", range(8))
@pytest.mark.parametrize("pose", POSE_IDS)
def test_quasi_set_log_likelihood_against_all_permutations(at_pose, pose, seed):
    xc.test_quasi_set_log_likelihood_against_all_permutations(seed)


@pytest.mark.parametrize("pose", POSE_IDS)
def test_measurement_model_against_second_reading(at_pose, pose):
    xc.test_measurement_model_against_second_reading()


@pytest.mark.parametrize("pose", POSE_IDS)
def test_measurement_model_behind_the_camera(pose):
    """MeasurePerfect and MeasurementJacobianL where the local depth is negative (Math.Sign, `mag`), and the detection
    probability there: the two readings on points behind a camera at every pose"""
    p = xc.prm3d_defaults(4, 600, 8)
    rng = np.random.default_rng(6)
    cam = np.concatenate([rng.uniform(-2, 2, 3), rigid.POSES[pose]])
    for local in np.concatenate([rigid.PLANT_BEHIND, rng.uniform(-1, 1, (8, 3)) * [1, 1, 0] - [0, 0, 1] * rng.uniform(0.05, 1.5, (8, 1))]):
        x = cam[:3] + rigid.rotation(cam[3:]) @ local
        z = xc.measure_perfect(p, cam, x)
        assert z[2] < 0
        assert np.allclose(orc.measure_perfect(p, cam, x), z, rtol=1e-12, atol=1e-12)
        assert np.allclose(orc.jacobian_l(p, cam, x), xc.jacobian_l(p, cam, x), rtol=1e-11, atol=1e-11)
        assert orc.detection_probability(p, cam, x) == 0 == xc.detection_probability_m(p, z)


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("pose", POSE_IDS)
def test_weight_alpha_against_second_reading(at_pose, pose, seed):
    xc.test_weight_alpha_against_second_reading(seed)


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("pose", POSE_IDS)
def test_prm3d_correct_against_second_reading(at_pose, pose, seed):
    xc.test_prm3d_correct_against_second_reading(seed)


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("pose", POSE_IDS)
def test_quasi_gradient_is_the_derivative_the_jacobian_describes(at_pose, pose, seed):
    xc.test_quasi_gradient_is_the_derivative_the_jacobian_describes(seed)


def test_transport_moves_what_a_particle_sees_nowhere():
    """transport against the oracle's own measurement model: from the moved pose, the moved map lies where it lay"""
    f = rigid.planted(2, 120, 32, rigid.FRAME_SEEDS[2, 120, 32])
    p = rigid.params(f)
    for name, q in rigid.POSES.items():
        g = rigid.transport(f, q)
        assert np.allclose(np.linalg.norm(g.poses[:, 3:], axis=1), np.linalg.norm(q))
        for i in range(f.P):
            a = np.array([orc.measure_perfect(p, f.poses[i], x) for x in f.mean[i]])
            b = np.array([orc.measure_perfect(p, g.poses[i], x) for x in g.mean[i]])
            assert np.allclose(a, b, rtol=1e-10, atol=1e-10), name


@pytest.mark.parametrize("P,C,M", rigid.ORACLE_FRAMES)
def test_oracle_is_invariant_under_rigid_transport(P, C, M):
    """predict / correct / prune / weight_alpha of a planted frame moved by every pose, mapped back, against the frame
    as it is"""
    f = rigid.planted(P, C, M, rigid.FRAME_SEEDS[P, C, M])
    p = rigid.params(f)
    rigid.assert_frame_bites(p, f)
    base = rigid.assert_frame_margins(p, f, what="(%d, %d, %d)" % (P, C, M))
    for name, q in rigid.POSES.items():
        g = rigid.transport(f, q)
        for i in range(P):
            what = "%s particle %d" % (name, i)
            moved = rigid.assert_margins(p, g.poses[i], g.z, g.map(i), what)
            rigid.assert_invariant(base[i], moved, q, what)


@pytest.mark.parametrize("case", list(rigid.STAGE_CASES))
def test_stage_inputs_bite_and_keep_their_margins(case):
    pose, C, M, env, timed, depth = rigid.STAGE_CASES[case]
    f = rigid.stage_frame(case)
    p = rigid.params(f)
    rigid.assert_frame_bites(p, f)
    d = biting_map(p, oracle_state(f, p.max_quantity), f.z, rigid.stage_seed(case), case) if depth else None
    with orc.depth_map(d):
        stages = rigid.assert_frame_margins(p, f, what=case)
        # a planted component of detection probability 0 is gated by a measurement, and every update from it weighs exactly 0
        for i in range(f.P):
            pred, cor = stages[i][0], stages[i][1]
            src, det = rigid.correct_sources(p, f.poses[i], f.z, pred)
            assert len(src) == len(cor[0])
            for j in rigid.zero_pd_planted(p, f, i):
                assert np.any(det & (src == j)) and np.all(cor[0][det & (src == j)] == 0), (case, i, j)
                assert cor[0][j] == f.w[i, j]


@pytest.mark.parametrize("case", list(rigid.STEP_CASES))
def test_step_inputs_bite_and_keep_their_margins(case):
    f = rigid.step_frame(case)
    p = rigid.params(f)
    rigid.assert_frame_bites(p, f)
    st = oracle_state(f, p.max_quantity)
    for s, (z, u) in enumerate(rigid.whole_step_inputs(f, rigid.step_seed(case))):
        what = "%s step %d" % (case, s)
        rigid.assert_state_margins(p, st, z, what)
        prior = st.weights.copy()
        _, _, _, alpha = orc.slam_update(p, st, z, u=u, threads=THREADS)
        rigid.assert_neff_margin(p, prior, alpha, what)


def test_turning_run_bites_and_keeps_its_margins():
    """the turning run of tests/test_gpu_rigid.py played by the oracle alone (the device's poses differ from
    orc.update_motion's by at most 1e-14, which the device test asserts; that moves a pixel by 1e-11 and a Mahalanobis
    distance, a weight or a density by less than 1e-9 relative, so the margins are asserted ten times as wide here: 1e-5
    and 1e-2): qw changes sign, every step keeps its margins"""
    f = rigid.turn_frame()
    p = rigid.params(f, max_measurements=rigid.TURN_MAX_M)
    rigid.assert_frame_bites(p, f)
    st = oracle_state(f, p.max_quantity)
    landmarks = rigid.turning_landmarks(f)
    qw, resampled, counts = [st.poses[0, 3]], 0, []
    for s, step in enumerate(rigid.turning_plan(f, rigid.TURN_SEED)):
        what = "%s step %d" % (rigid.TURN_CASE, s)
        st.poses[:] = orc.update_motion(st.poses, rigid.TURN_READING, step["noise"])
        z = rigid.turning_measurements(p, st.poses[0], landmarks, step)
        counts.append(len(z))
        rigid.assert_state_margins(p, st, z, what, scale=10)
        prior = st.weights.copy()
        _, _, res, alpha = orc.slam_update(p, st, z, u=step["u"], threads=THREADS)
        rigid.assert_neff_margin(p, prior, alpha, what, scale=10)
        resampled += int(res)
        qw.append(st.poses[0, 3])
    assert qw[0] > 0.3 and qw[-1] < -0.3 and any(abs(x) < 0.3 for x in qw), "qw along the run: %r" % (qw,)
    assert min(counts) > 20, "measurements per step: %r" % (counts,)
