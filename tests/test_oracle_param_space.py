"""The reference away from prm3d_defaults (tests/paramspace.py), on the host: the second readings of
tests/test_oracle_crosscheck.py run with each named parameter set instead of the defaults, at that file's own tolerances;
and every precondition of the frames tests/test_gpu_param_space.py hands the device — the planted layout bites for every
particle, no input sits on a discrete edge, and the set changes on the reference what it is there to change — so that
a set that does not bite is found without a GPU."""
import json
import os

import numpy as np
import pytest

import orc
import paramspace as ps
import test_oracle_crosscheck as xc
from monorfs_amd.abi import PHD_GATE_EUCLIDEAN, PHD_GATE_SQUARED_EUCLIDEAN, params_from_dict, prm3d_defaults

SETS = pytest.mark.parametrize("name", ps.PRM3D_SETS)


def case_for(rng, p, J, M):
    """test_oracle_crosscheck.random_case for p's camera: landmarks inside p's film and range clip, reaching into its ramp
    bands (a detection probability between 0 and PD); measurements next to some of them + N(0, R) by a Cholesky factor,
    and clutter"""
    c = ps.Camera(p)
    pose = np.concatenate([rng.normal(0, 0.05, 3), [1.0, 0.0, 0.0, 0.0] + rng.normal(0, 0.03, 4)])
    zs = np.column_stack([rng.uniform(c.left + 2, c.right - 2, J), rng.uniform(c.top + 2, c.bottom - 2, J),
                          rng.uniform(c.rmin + 0.05, c.rmax - 0.05, J)])
    lm = np.array([xc.measure_to_map(p, pose, zz) for zz in zs])
    L = np.linalg.cholesky(np.array(p.R).reshape(3, 3))
    z = []
    for k in range(M):
        if k < J and rng.uniform() < 0.8:
            z.append(zs[k] + 1.5 * L @ rng.normal(0, 1, 3))
        else:
            z.append([rng.uniform(c.left, c.right), rng.uniform(c.top, c.bottom), rng.uniform(c.rmin, c.rmax)])
    return pose, lm, np.array(z)


def block(name):
    return ps.params(name, P=4, M=8)


def field(p, name):
    v = getattr(p, name)
    return tuple(v) if hasattr(v, "_length_") else v


def test_the_sets_leave_the_defaults():
    """every set differs from prm3d_defaults in the fields it names, and in no other"""
    d = prm3d_defaults(4, 600, 8)
    for name in ps.PRM3D_SETS:
        p = block(name)
        changed = {f for f, _ in p._fields_ if field(p, f) != field(d, f)} - {"max_particles", "max_components", "max_measurements"}
        named = {{"focal": "measurer", "film": "measurer", "range_clip": "measurer"}.get(k, k) for k, v in ps.SETS[name].items()
                 if not (np.isscalar(v) and getattr(d, k, None) == v)}   # (a set may state a default: sq_*'s metric, small_minw_wide's cut)
        assert changed == named, (name, changed, named)
    R = np.array(block("correlated").R).reshape(3, 3)
    assert np.allclose(sorted(np.linalg.eigvalsh(R)), [1.6e-4, 0.13, 5.4], rtol=0.05)
    c = ps.Camera(block("camera"))
    assert (c.left, c.top, c.right, c.bottom) == (-200, -150, 300, 183)
    assert c.rmin != 0.3 and c.rmax != 3.1 and abs(c.rmin - 0.3) < 1e-7 and abs(c.rmax - 3.1) < 1e-6


@SETS
def test_prm3d_correct_against_second_reading(name):
    p = block(name)
    updates = 0
    for seed in range(4):
        w, n = xc.check_prm3d_correct(p, seed, case_for)
        updates += np.count_nonzero(w[n:] > 0)
    assert updates >= 4, "no detection update of positive weight: nothing of the innovation covariance was compared"


@SETS
def test_set_log_likelihood_against_all_permutations(name):
    p = block(name)
    got = [xc.check_set_log_likelihood(p, seed, case_for) for seed in range(12)]
    assert np.all(np.isfinite(got))


@SETS
def test_quasi_set_log_likelihood_against_all_permutations(name):
    p = block(name)
    got = [xc.check_quasi_set_log_likelihood(p, seed, case_for) for seed in range(8)]
    assert np.all(np.isfinite(got))


@SETS
def test_measurement_model_against_second_reading(name):
    xc.check_measurement_model(block(name), case_for)


@SETS
def test_weight_alpha_against_second_reading(name):
    p = block(name)
    assert sum(xc.check_weight_alpha(p, seed, case_for) for seed in range(6)) >= 4


@SETS
def test_quasi_gradient_is_the_derivative_the_jacobian_describes(name):
    p = block(name)
    g = [xc.check_quasi_gradient(p, seed, case_for) for seed in range(6)]
    assert np.max(np.abs(g)) > 1


def test_the_detection_probability_on_every_ramp_of_the_moved_camera():
    """the oracle against the numpy reading on the planted points of the camera set: every band, outside every side"""
    p = block("camera")
    pz, _ = ps.plant_points(p)
    got = orc.detection_probability_m(p, pz)
    want = np.array([xc.detection_probability_m(p, z) for z in pz])
    assert np.allclose(got, want, rtol=1e-12, atol=1e-15)
    assert np.all((got[:ps.NBAND] > 0) & (got[:ps.NBAND] < p.pd)) and np.all(got[ps.NBAND:] == 0)
    assert len({round(float(x), 6) for x in got[:ps.NBAND]}) == 1   # (the middle of every band: half of PD through three divisors)


def test_gate_rule_of_the_second_reading():
    """gate2 is make_dev_params' radius rule: the radius itself under the squared metric, its square under the Euclidean
    one, and today's behaviour at the defaults"""
    p = prm3d_defaults(1, 600, 8)
    assert xc.gate2(p) == p.density_distance_threshold == 0.5 and xc.gate2(p, 3) == 1.5
    for r in (0.2, 1.7):
        p.density_distance_threshold = r
        p.gate_metric = PHD_GATE_EUCLIDEAN
        assert xc.gate2(p) == r * r and xc.gate2(p, 3) == (3 * r) * (3 * r)
        p.gate_metric = PHD_GATE_SQUARED_EUCLIDEAN
        assert xc.gate2(p) == r and xc.gate2(p, 3) == 3 * r


# ---- Linear2D ---------------------------------------------------------------------------------------------------------
KAT = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "phdnavigator_kat.json")))


def linear2d_correct(p, pose2, z, pred):
    """CorrectConditional for the Linear2D toy model in numpy: z = landmark - pose (H = I on the first two coordinates), a
    2 x 2 R; the third coordinate is carried along"""
    R = np.array(p.R)[:4].reshape(2, 2)
    H = np.array([[1.0, 0, 0], [0, 1.0, 0]])
    out = [((1 - p.pd) * w, m, P) for w, m, P in zip(*pred)]   # (every landmark below is in full view)
    for zk in z:
        rows = []
        for w, m, P in zip(*pred):
            S = H @ P @ H.T + R
            d = zk - (m[:2] - pose2)
            K = P @ H.T @ np.linalg.inv(S)
            q = np.exp(-0.5 * d @ np.linalg.inv(S) @ d) / (2 * np.pi * np.sqrt(np.linalg.det(S)))
            rows.append((p.pd * w * q, m + K @ d, (np.eye(3) - K @ H) @ P))
        total = p.clutter_density + sum(r[0] for r in rows)
        out += [(r[0] / total, r[1], r[2]) for r in rows]
    return out


def test_linear2d_correct_with_a_correlated_R():
    from monorfs_amd.abi import PHD_GATE_DISABLED
    rng = np.random.default_rng(71)
    p = ps.linear2d_params(dict(KAT["params"], gate_metric=PHD_GATE_DISABLED))
    assert list(p.R)[:4] == [5e-4, 3e-4, 3e-4, 8e-4] and p.measurer[0] == 4.25
    lm = rng.uniform(-2, 2, (5, 2))
    A = rng.uniform(-0.05, 0.05, (5, 3, 3))
    pred = (rng.uniform(0.4, 1.1, 5), np.column_stack([lm, np.zeros(5)]), A @ A.transpose(0, 2, 1) + 1e-3 * np.eye(3))
    pose2 = np.array([0.1, -0.2])
    z = lm[:3] - pose2 + rng.multivariate_normal([0, 0], ps.LINEAR2D_R, 3)
    want = linear2d_correct(p, pose2, z, pred)
    ow, om, oc = orc.correct(p, list(pose2) + [0.0], z, pred)
    assert len(ow) == len(want)
    for i, (w, m, P) in enumerate(want):
        assert np.isclose(ow[i], w, rtol=1e-9, atol=1e-300), (i, ow[i], w)
        assert np.allclose(om[i], m, rtol=1e-9, atol=1e-12) and np.allclose(oc[i][:2, :2], P[:2, :2], rtol=1e-8, atol=1e-14)
    assert np.count_nonzero(ow[5:] > 0.1) >= 3
    diag = orc.correct(params_from_dict(dict(KAT["params"], gate_metric=PHD_GATE_DISABLED, measurer=[4.25], R=[[5e-4, 0], [0, 8e-4]])),
                       list(pose2) + [0.0], z, pred)[0]
    assert np.max(np.abs(diag - ow) / np.maximum(ow, 1e-300)) > 1e-3   # (the correlation moves the weights)


# ---- the frames of tests/test_gpu_param_space.py ---------------------------------------------------------------------
STAGE_IDS = [(name, shape) for name in ps.PRM3D_SETS for shape in ps.STAGE_SHAPES[name]]


@pytest.mark.parametrize("name,shape", STAGE_IDS, ids=["%s-P%d-C%d-M%d" % ((n,) + s) for n, s in STAGE_IDS])
def test_stage_frames_meet_their_preconditions(name, shape):
    ps.checked_frame(name, *shape, ps.stage_seed(name, shape))


STEP_IDS = [(name, shape) for name in ps.STEP_SETS for shape in ps.STEP_SHAPES]


@pytest.mark.parametrize("name,shape", STEP_IDS, ids=["%s-P%d-C%d-M%d" % ((n,) + s) for n, s in STEP_IDS])
def test_step_frames_meet_their_preconditions(name, shape):
    """the planted layout, the margins of every step's input state and of N_eff; with MinEffectiveParticle 0.6 (filter,
    all_of_it) one step must resample and one must not"""
    p, f, seed = ps.step_frame(name, shape)
    run = ps.oracle_steps(name, p, f, seed)
    res = [r[6] for r in run]
    if p.min_effective_particle == 0.6:
        assert True in res and False in res, "resampling decisions %r" % (res,)


def test_pd_one_frame_is_in_the_oracle_s_classes():
    """PD = 1: log(1 - PD) = -inf is the misdetection factor of every landmark in full view. On the reference the
    misdetection copy of such a component weighs (1 - PD) w = 0 and leaves the map, so a landmark of the map estimate in
    full view stems from a detection update and holds that measurement inside its gate: the set log-likelihood is finite
    for every particle of this frame, and never NaN; alpha is 0 exactly where it is -inf."""
    p, f, want = ps.pd_one_case()
    sll = np.array([w[4] for w in want])
    a = np.array([w[3] for w in want])
    assert not np.any(np.isnan(sll)) and not np.any(np.isnan(a))
    assert np.all((a == 0) == np.isneginf(sll))
    assert np.all(np.isfinite(sll)) and np.all(a > 0)
    for i, (pred, cor, _, _, _) in enumerate(want):   # (the copies of the components in full view are gone)
        pd = np.array([orc.detection_probability(p, f.poses[i], x) for x in pred[1]])
        assert np.count_nonzero(pd == 1.0) >= 10 and np.all(cor[0][:len(pd)][pd == 1.0] == 0)
