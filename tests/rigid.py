"""Rigid transport of synthetic frames, and the one table of cases the rigid tests run (tests/test_oracle_rigid.py on the
host, against the oracle alone; tests/test_gpu_rigid.py on the device).

monorfs_amd/synth.py draws every particle pose next to the identity and every prior component well inside the field of
view. `transport` moves a whole frame (map, particle poses) by a rigid motion: what the filter computes is the same up
to that motion, and the rotations R(q), R(q*), the pose Jacobians and the quaternion products are exercised at real
angles. `plant_edges` puts components into each of the six visibility ramp bands, outside the film, beyond both range
clips and behind the camera, and measurements into the bands. `assert_bites` shows on the oracle that a frame does
what it is planted for; `assert_margins` that none of its inputs sits on a discrete edge (the device's dense sums agree
with the oracle to about 1e-9 only, so a weight on MinWeight or a distance on a gate would make the comparison a coin toss).

A seed whose frame fails a margin at one of its poses is replaced by the next one HERE, as a literal (see FRAME_SEEDS),
never at run time."""
import copy

import numpy as np

import orc
from monorfs_amd.abi import prm3d_defaults
from monorfs_amd.synth import measure_to_map_identity
from test_gpu_shape_edges import frame, klass, path_of, perturbed
from test_oracle_crosscheck import gate2, multiplier

S = np.sqrt(0.5)
POSES = {   # unit quaternions (w, x, y, z), but for the last
    "x90": np.array([S, S, 0.0, 0.0]),
    "y90": np.array([S, 0.0, S, 0.0]),
    "z90": np.array([S, 0.0, 0.0, S]),
    "y180": np.array([0.0, 0.0, 1.0, 0.0]),                                                  # qw = 0
    "axes120": np.array([0.5, 0.5, 0.5, 0.5]),                                               # permutes the axes
    "generic-negw": np.array([-0.3, 0.6, -0.5, 0.55]) / np.linalg.norm([-0.3, 0.6, -0.5, 0.55]),
    "unnorm": np.array([1.1, -2.0, 0.7, 3.0]),                                               # handed over as it is
}
IDENTITY = np.array([1.0, 0.0, 0.0, 0.0])
TRANSLATION = np.array([1.3, -2.1, 0.7])


def qmul(a, b):
    """Hamilton product over the last axis (Quaternion.cs:295-301)"""
    a, b = np.asarray(a, float), np.asarray(b, float)
    aw, ax, ay, az = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bw, bx, by, bz = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([aw * bw - ax * bx - ay * by - az * bz,
                     aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw], axis=-1)


def rotation(q):
    """R(q / |q|): v -> q v q*"""
    w, x, y, z = np.asarray(q, float) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def move_points(x, q, t=TRANSLATION):
    return np.asarray(x, float) @ rotation(q).T + t


def move_covariances(c, q):
    R = rotation(q)
    return R @ np.asarray(c, float) @ R.T


def move_poses(poses, q, t=TRANSLATION):
    """poses[..., 7] (location, quaternion): location -> R t_i + t, quaternion -> q^ (x) q_i, times |q| (1 for a unit q:
    the product keeps the norm a caller hands over)"""
    poses = np.asarray(poses, float)
    n = np.linalg.norm(q)
    return np.concatenate([move_points(poses[..., :3], q, t), qmul(np.asarray(q, float) / n, poses[..., 3:]) * n], axis=-1)


def back_points(x, q, t=TRANSLATION):
    return (np.asarray(x, float) - t) @ rotation(q)


def back_covariances(c, q):
    R = rotation(q)
    return R.T @ np.asarray(c, float) @ R


def back_mixture(mix, q, t=TRANSLATION):
    w, m, c = mix
    return np.array(w), back_points(m, q, t).reshape(-1, 3), back_covariances(c, q).reshape(-1, 3, 3)


def transport(f, q, t=TRANSLATION):
    """a copy of the synth.Frame f moved by (q / |q|, t); measurements and weights stay"""
    g = copy.copy(f)
    g.mean = move_points(f.mean, q, t)
    g.cov = move_covariances(f.cov, q)
    g.poses = move_poses(f.poses, q, t)
    g.w, g.z, g.counts, g.weights = np.array(f.w), np.array(f.z), np.array(f.counts), np.array(f.weights)
    return g


# ---- the planted components -------------------------------------------------------------------------------------------
PLANT_Z = np.array([   # pixel-range points
    [317, 0, 1], [-318, 10, 1], [0, 237, 1], [5, -238, 1], [0, 0, 1.95], [0, 0, 0.15],   # one in each ramp band
    [330, 0, 1], [0, 0, 2.3], [100, 100, 0.05]], float)                                   # outside the film, beyond rmax, below rmin
PLANT_BEHIND = np.array([[0.1, 0.1, -0.5], [0.0, 0.2, -0.08]])                            # local points behind the camera
NPLANT = len(PLANT_Z) + len(PLANT_BEHIND)
PLANT_WEIGHT = 0.8
# What every particle of a frame must see of the layout (assert_bites), and what the first FULL_PARTICLES must.
# A particle stands 2.4 mm (one odometry-noise step) off the origin and its planted components 1 mm off their points:
# 1.5 px at 1 m, against the 1.24 px between pixel 317 and the inner end of its ramp band (320 - 4.24). A given
# particle has all four film-edge components inside their bands with probability 0.42 only, so a seed with ALL six ramp
# components on the ramp exists for four particles (one in 30; the stage and invariance frames have no more particles),
# not for 8 or 64. Every particle of every frame must still see the two range-band components and at least one film-edge
# component on a ramp (MIN_RAMP), all five PD = 0 components, two of them behind the camera, a measurement that gates a
# PD = 0 component with a ramp component, and a birth from a measurement in a band.
FULL_PARTICLES, FULL_RAMP, MIN_RAMP = 4, 6, 3


def plant_edges(f):
    """overwrites the first NPLANT components of every particle of f (built at the identity: before transport) and its
    measurements 0 - 5, in place; returns f"""
    assert f.C >= NPLANT and f.M >= 6
    rng = np.random.default_rng([977, f.P, f.C, f.M])
    f.mean, f.w, f.cov = np.array(f.mean), np.array(f.w), np.array(f.cov)
    base = np.concatenate([measure_to_map_identity(PLANT_Z), PLANT_BEHIND])
    f.mean[:, :NPLANT] = base[None] + rng.normal(size=(f.P, NPLANT, 3)) * 1e-3
    f.w[:, :NPLANT] = PLANT_WEIGHT
    f.z = np.array(f.z)
    f.z[0:4] = PLANT_Z[0:4] + [0.5, -0.5, 0.003]
    f.z[4] = [0, 0, 1.93]
    f.z[5] = [1, 1, 0.17]
    return f


def planted(P, C, M, seed, pose=None):
    """the frame of a case: test_gpu_shape_edges.frame (steady weights), planted, moved by POSES[pose] (None: as it is)"""
    f = plant_edges(frame(P, C, M, seed))
    return f if pose is None else transport(f, POSES[pose])


def params(f, maxq=600, max_measurements=None):
    """the parameters test_gpu_shape_edges.make gives a handle for f"""
    p = prm3d_defaults(max_particles=f.P, max_components=max(maxq, f.C), max_measurements=max_measurements or max(f.M, 1))
    p.max_quantity = maxq
    return p


def zero_pd_planted(p, f, i):
    """the planted components of particle i whose detection probability is exactly 0"""
    return [j for j in range(NPLANT) if orc.detection_probability(p, f.poses[i], f.mean[i, j]) == 0]


def correct_sources(p, pose, z, pred):
    """the predicted component each entry of orc.correct's result stems from, and whether it is a detection update:
    the misdetection copies in order, then per measurement the components within the gate (PHDNavigator.cs:837-903)"""
    n = len(pred[0])
    src, det = list(range(n)), [False] * n
    for zk in z:
        x = orc.measure_to_map(p, pose, zk)
        near = np.nonzero(np.sum((pred[1] - x) ** 2, axis=1) <= gate2(p))[0]
        src += list(near)
        det += [True] * len(near)
    return np.array(src), np.array(det)


def full_particles(f):
    return range(min(f.P, FULL_PARTICLES))


def assert_frame_bites(p, f):
    """assert_bites for EVERY particle of f: all six ramp components for the first FULL_PARTICLES, MIN_RAMP beyond"""
    for i in range(f.P):
        assert_bites(p, f, i, FULL_RAMP if i < FULL_PARTICLES else MIN_RAMP)


def assert_bites(p, f, i, nramp=FULL_RAMP):
    """on the oracle alone: particle i of f sees what plant_edges planted, with at least nramp components on a ramp"""
    pose = f.poses[i]
    w, m, c = f.map(i)
    zh = np.array([orc.measure_perfect(p, pose, x) for x in m])
    local = (m - pose[:3]) @ rotation(pose[3:])
    assert np.all(np.abs(local[:, 2]) >= 1e-3), "a component within 1e-3 of the camera plane: the reference divides by that depth"
    pd = np.array([orc.detection_probability(p, pose, x) for x in m])
    ramp, zero = (pd > 0) & (pd < p.pd), pd == 0
    assert np.count_nonzero(ramp) >= nramp, "%d components on a visibility ramp" % np.count_nonzero(ramp)
    assert np.count_nonzero(zero) >= 5 and np.count_nonzero(zero & (zh[:, 2] < 0)) >= 2, \
        "%d components at PD 0, %d of them behind the camera" % (np.count_nonzero(zero), np.count_nonzero(zero & (zh[:, 2] < 0)))
    both = 0
    for zk in f.z:
        near = np.sum((m - orc.measure_to_map(p, pose, zk)) ** 2, axis=1) <= gate2(p)
        both += bool(np.any(near & zero) and np.any(near & ramp))
    assert both >= 1, "no measurement gates a PD 0 component together with a ramp component"
    pred = orc.predict(p, pose, f.z, (w, m, c))
    zpd = orc.detection_probability_m(p, f.z)
    xs = np.array([orc.measure_to_map(p, pose, zk) for zk in f.z])
    born = [k for b in pred[1][len(w):] for k in np.nonzero((xs == b).all(axis=1))[0]]
    assert any(0 < zpd[k] < p.pd for k in born), "no birth from a measurement in a ramp band (births from %r)" % (born,)


def explored_density(p, pose, z, mix):
    """Map.Evaluate(x, 3 DensityDistanceThreshold) at the map point of every measurement (PHDNavigator.cs:956-959, the
    gate of Map.Near in p's metric: test_oracle_crosscheck.gate2)"""
    w, m, c = mix
    out = np.zeros(len(z))
    if len(w) == 0:
        return out
    mult = np.array([multiplier(ci) for ci in c])
    inv = np.linalg.inv(c)
    for k, zk in enumerate(z):
        d = orc.measure_to_map(p, pose, zk) - m
        near = np.sum(d * d, axis=1) <= gate2(p, 3)
        out[k] = np.sum((w * mult * np.exp(-0.5 * np.einsum("na,nab,nb->n", d, inv, d)))[near])
    return out


def off(x, edge, rel):
    """every x is farther than rel * edge from edge"""
    return bool(np.all(np.abs(np.asarray(x, float) - edge) > rel * edge))


def assert_gate_margins(p, pose, z, mix, pred, what="", scale=1.0):
    """no squared distance between a measurement's map point and a component on the gate of the correction (the predicted
    components) or of the explored density (the prior ones, three radii), 1e-9 relative: test_oracle_crosscheck.gate2"""
    for means, factor, name in ((pred[1], 1, "correction"), (mix[1], 3, "exploration")):
        g = gate2(p, factor)
        if len(means) == 0 or not np.isfinite(g):
            continue
        for zk in z:
            d2 = np.sum((means - orc.measure_to_map(p, pose, zk)) ** 2, axis=1)
            assert off(d2, g, 1e-9 * scale), "%s: a distance on the %s gate" % (what, name)


def assert_margins(p, pose, z, mix, what="", scale=1.0, exempt=()):
    """no input of one particle's stages on a discrete edge, on the oracle's numbers: corrected weights against MinWeight,
    the explored density against ExplorationThreshold, the Mahalanobis distances of the set log-likelihood against its
    gate of 5 (all 1e-6; 1e-6 relative for the first two; times `scale`), the gated distances against the gate of p's
    metric (assert_gate_margins). exempt: indices into the corrected mixture that the MinWeight margin leaves out (entries
    a frame plants ON MinWeight). Returns the oracle's (predicted, corrected, pruned, alpha, set log-likelihood)."""
    assert off(explored_density(p, pose, z, mix), p.exploration_threshold, 1e-6 * scale), what + ": an explored density on ExplorationThreshold"
    pred = orc.predict(p, pose, z, mix)
    assert_gate_margins(p, pose, z, mix, pred, what, scale)
    cor = orc.correct(p, pose, z, pred)
    checked = np.delete(cor[0], np.asarray(exempt, int)) if len(exempt) else cor[0]
    assert off(checked, p.min_weight, 1e-6 * scale), what + ": a corrected weight on MinWeight"
    pr = orc.prune(p, cor)
    lm, _ = orc.best_map_estimate(pr)
    if len(lm) and len(z):
        zh = np.array([orc.measure_perfect(p, pose, x) for x in lm])
        d = zh[:, None, :] - np.asarray(z)[None, :, :]
        Rinv = np.linalg.inv(np.array(p.R).reshape(3, 3))
        maha = np.sqrt(np.einsum("jka,ab,jkb->jk", d, Rinv, d))
        assert np.all(np.abs(maha - 5) > 1e-6 * scale), what + ": a Mahalanobis distance on the association gate"
    a, sll = orc.weight_alpha(p, pose, z, pred, pr)
    assert np.isfinite(sll) and np.isfinite(a), what + ": set log-likelihood %r, alpha %r" % (sll, a)
    return pred, cor, pr, a, sll


def assert_frame_margins(p, f, z=None, what=""):
    z = f.z if z is None else z
    return [assert_margins(p, f.poses[i], z, f.map(i), "%s particle %d" % (what, i)) for i in range(f.P)]


def assert_state_margins(p, st, z, what="", scale=1.0):
    for i in range(st.P):
        assert_margins(p, st.poses[i], z, st.map(i), "%s particle %d" % (what, i), scale)


def assert_neff_margin(p, prior_weights, alpha, what="", scale=1.0):
    """N_eff / P of the weights a step resamples on, against MinEffectiveParticle (1e-3 relative)"""
    w = np.asarray(prior_weights) * np.asarray(alpha)
    s = w.sum()
    w = w / (s if s != 0 else 1)
    neff = 1.0 / np.sum(w * w) / len(w)
    assert off(neff, p.min_effective_particle, 1e-3 * scale), "%s: N_eff / P = %r on MinEffectiveParticle" % (what, neff)


def whole_step_inputs(f, seed, nsteps=3):
    """the measurements and u of test_gpu_shape_edges.whole_steps without a depth map, step by step"""
    rng = np.random.default_rng(seed)
    out = []
    for s in range(nsteps):
        z = perturbed(f.z, rng, 0.2 * s)
        out.append((z, float(rng.uniform(0.05, 0.95))))
    return out


# ---- the turning trajectory -------------------------------------------------------------------------------------------
TURN_STEPS = 6
TURN_READING = np.array([0.0, 0.0, 0.05, 0.0, 0.55, 0.0])   # 0.05 m forward, 0.55 rad yaw: 3.3 rad over the run, qw changes sign
TURN_MAX_M = 256


def turning_landmarks(f):
    """what the camera measures along the run: the landmarks of particle 0's map (planted ones included), and a copy of
    them for every step, carried along with the noise-free motion — the camera after k steps faces copy k as it faced the
    map at the start, and sees parts of the copies next to it"""
    pose = f.poses[0].copy()
    R0, out = rotation(pose[3:]), [f.mean[0].copy()]
    for _ in range(TURN_STEPS):
        pose = orc.update_motion(pose[None], TURN_READING)[0]
        out.append((f.mean[0] - f.poses[0, :3]) @ (rotation(pose[3:]) @ R0.T).T + pose[:3])
    return np.concatenate(out)


def turning_plan(f, seed):
    """the random numbers of the turning run, drawn up front: per step the odometry noise of every particle, which
    landmarks are measured (nine in ten of those that weigh more than 0.5 in the map, the steady profile's detected
    ones, and the planted ones, of every copy), their measurement noise, clutter and u"""
    rng = np.random.default_rng(seed)
    n = f.C * (TURN_STEPS + 1)
    plan = []
    for _ in range(TURN_STEPS):
        plan.append(dict(noise=rng.normal(size=(f.P, 6)) * np.sqrt([5e-3] * 3 + [2e-4] * 3) / 30,
                         pick=(np.tile(f.w[0] > 0.5, TURN_STEPS + 1) & (rng.uniform(size=n) < 0.9)) | (np.arange(n) % f.C < NPLANT),
                         znoise=rng.normal(size=(n, 3)) * np.sqrt([2.0, 2.0, 1e-3]),
                         clutter=np.stack([rng.uniform(-320, 320, 5), rng.uniform(-240, 240, 5), rng.uniform(0.25, 2.0, 5)], axis=1),
                         u=float(rng.uniform(0.05, 0.95))))
    return plan


def turning_measurements(p, pose, landmarks, step):
    """what the camera at `pose` measures of the picked `landmarks` where the oracle's detection probability is
    positive: the numpy MeasurePerfect + N(0, R), then the step's clutter"""
    from test_oracle_crosscheck import measure_perfect
    z = [measure_perfect(p, pose, x) + step["znoise"][j] for j, x in enumerate(landmarks)
         if step["pick"][j] and orc.detection_probability(p, pose, x) > 0]
    assert len(z) + len(step["clutter"]) <= TURN_MAX_M
    return np.array(z + list(step["clutter"]))


# ---- the table --------------------------------------------------------------------------------------------------------
# The seed of the frame of every (P, C, M) the tests use: the first from its starting value (5, 6, 7100, 7200, ... 7700)
# whose planted frame bites (about one seed in a hundred does: four particles with every film-edge component inside its
# band, and a measurement in a band that nothing explains) and keeps every margin at every pose it is used with. No seed
# that bit failed a margin. tests/test_oracle_rigid.py states both for the seeds below.
FRAME_SEEDS = {
    (2, 120, 32): 152, (2, 130, 70): 15,                                                # the oracle's invariance
    (4, 120, 32): 7827, (4, 120, 64): 7252, (4, 120, 128): 7353, (4, 120, 256): 7407, (4, 130, 64): 7647,
    (8, 120, 32): 7851, (64, 120, 64): 7775,                                           # whole steps, the turning run
}
CHAIN, SEPARATE = {}, {"PHD_CHAIN_MAX": "0"}


def _stage_id(pose, C, M, env, extra=""):
    c = "" if C == 120 else "C%d-" % C
    return "%s-%sM%d-%s%s-%s" % (pose, c, M, klass(M), extra, path_of(4, M, env))


# id -> (pose or None, C, M, environment at phd_create, timed, depth)
STAGE_CASES = {}
for _pose in POSES:
    for _M, _env in ((32, CHAIN), (64, SEPARATE)):
        STAGE_CASES[_stage_id(_pose, 120, _M, _env)] = (_pose, 120, _M, _env, False, False)
for _M in (128, 256):
    for _env in (CHAIN, SEPARATE):
        STAGE_CASES[_stage_id("generic-negw", 120, _M, _env)] = ("generic-negw", 120, _M, _env, False, False)
for _env in (CHAIN, SEPARATE):
    STAGE_CASES[_stage_id("generic-negw", 130, 64, _env)] = ("generic-negw", 130, 64, _env, False, False)
for _M in (32, 128):
    STAGE_CASES[_stage_id("generic-negw", 120, _M, CHAIN, "-timed")] = ("generic-negw", 120, _M, CHAIN, True, False)
for _M in (32, 64):
    STAGE_CASES[_stage_id("generic-negw", 120, _M, CHAIN, "-depth")] = ("generic-negw", 120, _M, CHAIN, False, True)
for _M, _env in ((32, CHAIN), (64, SEPARATE)):
    STAGE_CASES[_stage_id("identity", 120, _M, _env)] = (None, 120, _M, _env, False, False)

# id -> (pose, P, M, environment)
STEP_CASES = {
    "x90-P8-M32-half-chain": ("x90", 8, 32, CHAIN),
    "y180-P8-M32-half-chain": ("y180", 8, 32, CHAIN),
    "generic-negw-P8-M32-half-chain": ("generic-negw", 8, 32, CHAIN),
    "axes120-P64-M64-zb1-separate-fused": ("axes120", 64, 64, SEPARATE),
}
for _id, (_pose, _P, _M, _env) in STEP_CASES.items():
    assert _id.endswith("%s-%s" % (klass(_M), path_of(_P, _M, _env)))

TURN_CASE = "turning-y90-P8-chain"    # the turning run starts from the frame (8, 120, 32) at y90: the yaw adds to its angle
TURN_POSE = "y90"
INVARIANCE_POSES = ["generic-negw", "y180"]     # device against device, M = 32 and 64
ORACLE_FRAMES = [(2, 120, 32), (2, 130, 70)]


def stage_frame(case):
    pose, C, M, env, timed, depth = STAGE_CASES[case]
    return planted(4, C, M, FRAME_SEEDS[4, C, M], pose)


def step_frame(case):
    pose, P, M, env = STEP_CASES[case]
    return planted(P, 120, M, FRAME_SEEDS[P, 120, M], pose)


def step_seed(case):
    return 8000 + list(STEP_CASES).index(case)


def turn_frame():
    return planted(8, 120, 32, FRAME_SEEDS[8, 120, 32], TURN_POSE)


TURN_SEED = 8100


def stage_seed(case):
    """the seed of a stage case's depth map (test_gpu_shape_edges.biting_map)"""
    return 7900 + list(STAGE_CASES).index(case)


def assert_invariant(base, moved, q, what, corrected_in_order=True):
    """the stages (predicted, corrected, pruned, alpha, set log-likelihood) of a frame moved by q, mapped back, against
    those of the frame itself: SURVEY 8d's tolerances as tests/test_gpu_parity.py applies them"""
    from test_gpu_parity import assert_mix_close, match_unordered
    pred0, cor0, pr0, a0, sll0 = base
    pred, cor, pr, a, sll = moved
    assert_mix_close(back_mixture(pred, q), pred0, 1e-9, what + ": predict")
    if corrected_in_order:
        assert_mix_close(back_mixture(cor, q), cor0, 1e-9, what + ": correct")
    else:
        match_unordered(back_mixture(cor, q), cor0, 1e-9)
    assert_mix_close(back_mixture(pr, q), pr0, 1e-7, what + ": prune")
    assert np.isfinite(sll0) and np.isclose(sll, sll0, rtol=1e-9, atol=1e-9), "%s: set log-likelihood %r vs %r" % (what, sll, sll0)
    assert np.isfinite(a0) and np.isclose(a, a0, rtol=1e-6, atol=0), "%s: alpha %r vs %r" % (what, a, a0)


# ---- the quasi batch --------------------------------------------------------------------------------------------------
# id -> (pose, J, M, the seed of test_gpu_parity's gradient batch at that shape); 300 landmarks lie in the HBM slab, beyond LDS
QUASI_CASES = {"%s-J%d-M%d-%s-%s" % (pose, J, M, klass(M), "lds" if J <= 256 else "hbm-slab"): (pose, J, M, seed)
               for J, M, seed, poses in ((40, 30, 182, list(POSES)), (300, 64, 184, ["generic-negw", "y180"])) for pose in poses}


def quasi_batch(case):
    """the batch of test_gpu_parity.test_quasi_set_log_likelihood_batch / _gradient_batch (48 candidate poses around the
    camera, two measurements crowding one landmark) with the landmarks and the poses moved by the case's pose: (frame,
    landmarks, measurements, poses)"""
    from monorfs_amd.synth import Frame
    pose, J, M, seed = QUASI_CASES[case]
    q = POSES[pose]
    rng = np.random.default_rng(seed)
    f = Frame(48, J, M, seed, weight_profile="steady")
    z = f.z[:M].copy()
    z[1] = z[0] + [3.0, -2.0, 0.01]
    z[2] = z[0] + [-4.0, 1.0, -0.02]
    poses = f.poses.copy()
    poses[:, :3] += rng.normal(0, 5e-3, (f.P, 3))
    poses[:, 3:] += rng.normal(0, 2e-3, (f.P, 4))
    return f, move_points(f.mean[0, :J], q), z, move_poses(poses, q)
