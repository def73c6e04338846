"""Named points of parameter space away from prm3d_defaults, frames made for them, and what a frame must show on the
oracle before the device is asked anything (tests/test_oracle_param_space.py on the host, tests/test_gpu_param_space.py
on the device).

Every step kernel reads `phd_params` through DevParams (make_dev_params, monorfs_amd/csrc/phdhip.hip): a hand-picked
upper triangle of the birth covariance, R and its inverse in the innovation covariance and in five copies of the
association entry, a film rectangle truncated to integers, a range clip rounded to float32, three ramp divisors, gate
radii that are r or r * r by metric, weight histograms counted from MinWeight's bit pattern. A diagonal R, an isotropic
birth covariance, a symmetric integer film and a radius of 0.5 hide a wrong index, a transposition or a swapped pair in
every one of them. SETS names the points; `params(name, f)` makes the parameter block of a frame, `frame_for` a frame
whose landmarks, measurements and planted edge components live inside THAT block's film and range clip.

synth.Frame draws for the default camera and stays as it is (bench.py's inputs come from it)."""
import numpy as np

import orc
import rigid
from monorfs_amd.abi import (PHD_GATE_EUCLIDEAN, PHD_GATE_SQUARED_EUCLIDEAN, kinect_defaults, params_from_dict,
                             prm3d_defaults)
from monorfs_amd.synth import Frame
from test_oracle_crosscheck import gate2, measure_perfect, measure_to_map


def covariance(variances, correlations):
    """D C D for the variances (x, y, r) and the correlations (xy, xr, yr); positive definite or it raises"""
    d = np.sqrt(np.asarray(variances, float))
    xy, xr, yr = correlations
    c = np.array([[1.0, xy, xr], [xy, 1.0, yr], [xr, yr, 1.0]])
    m = d[:, None] * c * d[None, :]
    m = 0.5 * (m + m.T)
    assert np.array_equal(m, m.T) and np.all(np.linalg.eigvalsh(m) > 0), "not positive definite: %r" % (np.linalg.eigvalsh(m),)
    return m


# eigenvalues 1.6e-4, 0.13, 5.4: ill-conditioned enough to show a wrong entry of R or of its inverse, and the oracle still
# agrees with the numpy reading at the tolerances of tests/test_oracle_crosscheck.py (tests/test_oracle_param_space.py)
R_CORRELATED = covariance((2.0, 3.5, 1e-3), (0.95, -0.9, -0.8))
BIRTH_CORRELATED = covariance((1e-2, 4e-3, 2.5e-2), (0.7, -0.5, 0.2))
# (the triple (0.8, -0.6, 0.3) is NOT positive definite: correlations are not picked by eye)
assert np.min(np.linalg.eigvalsh(np.array([[1, 0.8, -0.6], [0.8, 1, 0.3], [-0.6, 0.3, 1.0]]))) < 0

CORRELATED = {"R": R_CORRELATED, "birth_covariance": BIRTH_CORRELATED}
# truncates to left -200, top -150, right 300, bottom 183: off the axis on both sides; neither range is a float32 value
CAMERA = {"focal": 410.5, "film": (-200.7, -150.2, 500.9, 333.3), "range_clip": (0.3, 3.1), "visibility_ramp": (11.0, 7.0, 0.3)}
FILTER = {"pd": 0.63, "clutter_density": 2e-5, "birth_weight": 0.3, "min_weight": 0.02, "merge_threshold": 1.5,
          "exploration_threshold": 1e-2, "max_quantity": 40, "min_effective_particle": 0.6}

SETS = {
    "correlated": CORRELATED,
    "camera": CAMERA,
    "filter": FILTER,
    # every weight of a map in the last bin of the histograms counted from MinWeight's bit pattern; the cut is active
    "small_minw": {"min_weight": 1e-12, "max_quantity": 40},
    # ... and the map estimate of alpha_assoc_body ranks hundreds of entries inside that one bin
    "small_minw_wide": {"min_weight": 1e-12, "max_quantity": 600},
    # a power of two: a bin edge ON MinWeight; births (PD 0: their copy keeps the weight) and the misdetection copies of
    # weight-0.5 components at PD 0.5 sit on it exactly, and `!(w < minw)` keeps them
    "large_minw": {"min_weight": 0.25, "birth_weight": 0.25, "pd": 0.5},
    "euclid_small": {"gate_metric": PHD_GATE_EUCLIDEAN, "density_distance_threshold": 0.2},
    "euclid_large": {"gate_metric": PHD_GATE_EUCLIDEAN, "density_distance_threshold": 1.7},
    "sq_small": {"gate_metric": PHD_GATE_SQUARED_EUCLIDEAN, "density_distance_threshold": 0.05},
    "sq_large": {"gate_metric": PHD_GATE_SQUARED_EUCLIDEAN, "density_distance_threshold": 2.0},
    "all_of_it": dict(CORRELATED, **dict(CAMERA, **FILTER)),
}
PRM3D_SETS = list(SETS)
LINEAR2D_R = [[5e-4, 3e-4], [3e-4, 8e-4]]
LINEAR2D_RANGE = 4.25
# overrides of the Linear2D parameters of tests/golden/phdnavigator_kat.json (linear2d_params)
LINEAR2D_SETS = {"linear2d_correlated": {"R": LINEAR2D_R, "measurer": [LINEAR2D_RANGE]}}


def apply(p, over):
    """the overrides of a set written into a parameter block; returns it"""
    for k, v in over.items():
        if k == "focal":
            p.measurer[0] = v
        elif k == "range_clip":
            p.measurer[1], p.measurer[2] = v
        elif k == "film":
            p.measurer[3], p.measurer[4], p.measurer[5], p.measurer[6] = v
        elif k in ("R", "birth_covariance"):
            getattr(p, k)[:] = [float(x) for x in np.asarray(v, float).reshape(9)]
        elif k == "visibility_ramp":
            p.visibility_ramp[:] = list(v)
        else:
            setattr(p, k, v)
    return p


def params(name, f=None, maxq=None, P=1, M=64, C=0, **more):
    """prm3d_defaults with the overrides of SETS[name] (and `more`), sized for the frame f; maxq: MaxQuantity where the set
    leaves it alone (600 otherwise)"""
    if f is not None:
        P, C, M = f.P, f.C, f.M
    over = dict(SETS[name], **more)
    q = over.get("max_quantity", 600 if maxq is None else maxq)
    p = prm3d_defaults(max_particles=P, max_components=max(600, q, C), max_measurements=max(M, 1))
    p.max_quantity = q
    return apply(p, over)


def kinect_params(name, P, M, delta=4):
    """kinect_defaults with the overrides of SETS[name]; returns (params, (resx, resy))"""
    p, res = kinect_defaults(P, 600, max(M, 1), delta)
    return apply(p, SETS[name]), res


def linear2d_params(kat_params, name="linear2d_correlated", **caps):
    """the Linear2D parameters of tests/golden/phdnavigator_kat.json with the overrides of LINEAR2D_SETS[name]: a
    correlated 2 x 2 R and another range"""
    return params_from_dict(dict(kat_params, **LINEAR2D_SETS[name]), **caps)


def with_R(p, R):
    """a copy of p with another R"""
    q = type(p).from_buffer_copy(p)
    q.R[:] = [float(x) for x in np.asarray(R, float).reshape(9)]
    return q


# ---- the camera of a parameter block ---------------------------------------------------------------------------------
class Camera:
    """what the measurer makes of p: the integer film rectangle, the float32 range clip, the ramps"""

    def __init__(self, p):
        self.left, self.top = int(p.measurer[3]), int(p.measurer[4])
        self.right, self.bottom = self.left + int(p.measurer[5]), self.top + int(p.measurer[6])
        self.rmin, self.rmax = float(np.float32(p.measurer[1])), float(np.float32(p.measurer[2]))
        self.ramp = [float(r) for r in p.visibility_ramp]
        self.cx, self.cy = 0.5 * (self.left + self.right), 0.5 * (self.top + self.bottom)


IDENTITY = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
BANDS = ["right", "left", "bottom", "top", "far", "near"]
NBAND = 6


def plant_points(p):
    """pixel-range points: one in the middle of each of the six ramp bands of p's rectangle and clip (BANDS, away from each
    other and at 0.8 of the far clip, where one odometry-noise step moves a pixel least), then one outside each film side,
    one beyond each range clip and a twin of the first of these; and two local points behind the camera"""
    c = Camera(p)
    hx, hy, hr = 0.5 * c.ramp[0], 0.5 * c.ramp[1], 0.5 * c.ramp[2]
    w, h = c.right - c.left, c.bottom - c.top
    far = c.rmin + 0.8 * (c.rmax - c.rmin)
    mid = c.rmin + 0.5 * (c.rmax - c.rmin)
    band = [[c.right - hx, c.cy + 0.1 * h, far], [c.left + hx, c.cy + 0.2 * h, far], [c.cx + 0.1 * w, c.bottom - hy, far],
            [c.cx - 0.1 * w, c.top + hy, far], [c.cx + 0.25 * w, c.cy + 0.25 * h, c.rmax - hr], [c.cx + 0.3 * w, c.cy - 0.2 * h, c.rmin + hr]]
    out = [[c.right + 3 * c.ramp[0], c.cy, mid], [c.left - 3 * c.ramp[0], c.cy, mid], [c.cx, c.bottom + 3 * c.ramp[1], mid],
           [c.cx, c.top - 3 * c.ramp[1], mid], [c.cx - 0.2 * w, c.cy - 0.25 * h, c.rmax + 3 * c.ramp[2]],
           [c.cx + 0.35 * w, c.cy + 0.3 * h, max(0.5 * c.rmin, c.rmin - 3 * c.ramp[2])],
           [c.right + 3 * c.ramp[0] + 0.3, c.cy, mid]]   # half a millimetre from the first of these: PruneModel merges the two
    return np.array(band + out, float), rigid.PLANT_BEHIND.copy()


NPLANT = 13 + len(rigid.PLANT_BEHIND)
PLANT_WEIGHT = rigid.PLANT_WEIGHT
TWINS = [NBAND, 12]   # the component outside the right film side and its twin
# measurement slots frame_for plants: one next to each band component, then a lone one in a band (it is born), then, for
# large_minw, a lone one outside the film (born at detection probability 0)
Z_BIRTH, Z_OUTSIDE = NBAND, NBAND + 1
NPLANT_Z = NBAND + 2
# large_minw: the prior components of weight 0.5, in full view and far from every measurement
ON_CUT = [NPLANT, NPLANT + 1, NPLANT + 2]
# the drawn landmarks keep to ranges beyond rmin + LANDMARKS_FROM * (rmax - rmin): the lone measurement in the near range
# band has nothing drawn within 0.7 m (a map of a few hundred components fills the frustum: a lone measurement among them
# is explained by some tail and not born)
LANDMARKS_FROM = 0.4


def local_to_map(pose, x):
    return np.asarray(pose[:3], float) + rigid.rotation(pose[3:]) @ np.asarray(x, float)


def lone_points(p):
    """the pixel-range points of the lone planted measurements and of the ON_CUT components"""
    c = Camera(p)
    w, h = c.right - c.left, c.bottom - c.top
    birth = np.array([c.cx - 0.25 * w, c.cy + 0.2 * h, c.rmin + 0.5 * c.ramp[2]])        # in the near range band
    outside = np.array([c.cx - 0.3 * w, c.cy + 0.3 * h, c.rmax + 0.6])                    # beyond the far clip
    far = c.rmin + 0.75 * (c.rmax - c.rmin)
    cut = np.array([[c.right - 0.15 * w, c.bottom - 0.15 * h, far], [c.right - 0.3 * w, c.bottom - 0.15 * h, 0.6 * far],
                    [c.right - 0.12 * w, c.cy - 0.1 * h, 0.5 * far]])
    return birth, outside, cut


def frame_for(p, P, C, M, seed, profile="steady", on_cut=False, spread=1.0):
    """A synth.Frame for p's camera: the draws of synth.Frame (poses one odometry-noise step off the identity, covariances,
    the two weight profiles), the landmarks uniform inside p's film, three ramps and three standard deviations off its
    sides, and in the far part of its range clip (LANDMARKS_FROM); nine measurements in ten are detections through the
    numpy measurement model + N(0, R) by a Cholesky factor of p's R, the others clutter uniform in the film. Per particle,
    seen from ITS pose: components in each of the six ramp bands, outside each film side, beyond both range clips and
    behind the camera (plant_points), a measurement next to each band component, a lone measurement in the near range band
    and one beyond the far clip. on_cut: the three ON_CUT components weigh 0.5 (large_minw). spread: scales how far the
    particles stand from each other and their maps differ (1: one odometry-noise step and 1e-2; a small one: a converged
    filter, whose particles weigh about the same)."""
    assert C >= NPLANT + len(ON_CUT) and M >= NPLANT_Z + 2
    rng = np.random.default_rng([seed, 0x9a7a])
    c = Camera(p)
    R = np.array(p.R).reshape(3, 3)
    L = np.linalg.cholesky(R)
    sd = np.sqrt(np.diag(R))
    f = Frame.__new__(Frame)
    f.P, f.C, f.M = P, C, M
    dt = 1.0 / 30
    dloc = rng.normal(size=(P, 3)) * np.sqrt(5e-3) * dt * spread
    drot = rng.normal(size=(P, 3)) * np.sqrt(2e-4) * dt * spread
    q = np.concatenate([np.ones((P, 1)), 0.5 * drot], axis=1)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    f.poses = np.concatenate([dloc, q], axis=1)
    birth, outside, cut = lone_points(p)
    span = c.rmax - c.rmin
    mx, my, mr = 3 * c.ramp[0] + 3 * sd[0], 3 * c.ramp[1] + 3 * sd[1], 2 * c.ramp[2] + 3 * sd[2]

    def draw(n, clutter=False):
        if clutter:
            return np.stack([rng.uniform(c.left, c.right, n), rng.uniform(c.top, c.bottom, n), rng.uniform(c.rmin + mr, c.rmax, n)], axis=1)
        return np.stack([rng.uniform(c.left + mx, c.right - mx, n), rng.uniform(c.top + my, c.bottom - my, n),
                         rng.uniform(c.rmin + LANDMARKS_FROM * span, c.rmax - mr, n)], axis=1)

    zc = draw(C)
    base = np.array([measure_to_map(p, IDENTITY, zz) for zz in zc])
    A = rng.uniform(-0.05, 0.05, size=(C, 3, 3))
    cov = A @ np.transpose(A, (0, 2, 1)) + 1e-4 * np.eye(3)
    f.mean = base[None] + rng.normal(size=(P, C, 3)) * 1e-2 * spread
    f.cov = np.array(np.broadcast_to(cov, (P, C, 3, 3)))
    f.counts = np.full(P, C, np.int32)
    f.weights = np.full(P, 1.0 / P)
    first = NPLANT + len(ON_CUT)
    nd = min(int(np.ceil(0.9 * (M - NPLANT_Z))), C - first)
    pick = first + rng.choice(C - first, size=nd, replace=False)
    zdet = np.array([measure_perfect(p, IDENTITY, base[j]) for j in pick]) + rng.normal(size=(nd, 3)) @ L.T
    zclu = draw(M - NPLANT_Z - nd, clutter=True).reshape(-1, 3)
    zfree = np.concatenate([zdet, zclu])[rng.permutation(M - NPLANT_Z)]
    if profile == "steady":
        w = rng.uniform(0.002, 0.06, C)
        w[pick] = rng.uniform(0.6, 1.2, nd)
    elif profile == "survey":
        w = rng.uniform(0.05, 1.2, C)
    else:
        raise ValueError("unknown weight profile %r" % (profile,))
    # ---- the planted components, per particle from ITS pose ----
    pz, behind = plant_points(p)
    w[:NPLANT] = PLANT_WEIGHT
    w[TWINS] = 1.3   # (above every drawn weight: the pair is inside any MaxQuantity cut)
    for i in range(P):
        for j, zz in enumerate(pz):
            f.mean[i, j] = measure_to_map(p, f.poses[i], zz)
        for j, x in enumerate(behind):
            f.mean[i, len(pz) + j] = local_to_map(f.poses[i], x)
        for j, zz in enumerate(cut):
            f.mean[i, NPLANT + j] = measure_to_map(p, f.poses[i], zz)
    f.mean[:, :first] += rng.normal(size=(P, first, 3)) * 1e-4
    f.cov[:, :first] = 0.005 * f.cov[:, :first] + 2.5e-5 * np.eye(3)   # (tight: the planted ones explain their own spot only)
    w[NPLANT:first] = 0.5 if on_cut else rng.uniform(0.3, 0.45, len(ON_CUT))
    f.w = np.array(np.broadcast_to(w, (P, C)))
    znext = pz[:NBAND] + np.array([0.1 * c.ramp[0], -0.1 * c.ramp[1], 0.03 * c.ramp[2]])
    f.z = np.concatenate([znext, [birth], [outside], zfree])
    return f


# ---- preconditions, on the oracle and numpy alone --------------------------------------------------------------------
def moved_sides(name):
    """the film sides a set moves: each must hold a component on its ramp"""
    return BANDS[:4] if "film" in SETS.get(name, {}) else []


def assert_bites(p, f, i, sides=()):
    """the analogue of rigid.assert_bites for p's rectangle, on particle i: at least 3 components with 0 < PD < pd, one on
    the ramp of every side in `sides`, one in each range band, at least 5 at PD 0 (two behind the camera), and a birth from
    a measurement in a band"""
    pose = f.poses[i]
    w, m, c = f.map(i)
    cam = Camera(p)
    zh = np.array([orc.measure_perfect(p, pose, x) for x in m])
    local = (m - pose[:3]) @ rigid.rotation(pose[3:])
    assert np.all(np.abs(local[:, 2]) >= 1e-3), "a component within 1e-3 of the camera plane"
    pd = np.array([orc.detection_probability(p, pose, x) for x in m])
    ramp, zero = (pd > 0) & (pd < p.pd), pd == 0
    assert np.count_nonzero(ramp) >= 3, "%d components on a visibility ramp" % np.count_nonzero(ramp)
    inside = (zh[:, 2] > cam.rmin + cam.ramp[2]) & (zh[:, 2] < cam.rmax - cam.ramp[2])
    xin = (zh[:, 0] > cam.left + cam.ramp[0]) & (zh[:, 0] < cam.right - cam.ramp[0])
    yin = (zh[:, 1] > cam.top + cam.ramp[1]) & (zh[:, 1] < cam.bottom - cam.ramp[1])
    on = {"right": ramp & inside & yin & (zh[:, 0] > cam.right - cam.ramp[0]), "left": ramp & inside & yin & (zh[:, 0] < cam.left + cam.ramp[0]),
          "bottom": ramp & inside & xin & (zh[:, 1] > cam.bottom - cam.ramp[1]), "top": ramp & inside & xin & (zh[:, 1] < cam.top + cam.ramp[1]),
          "far": ramp & xin & yin & (zh[:, 2] > cam.rmax - cam.ramp[2]), "near": ramp & xin & yin & (zh[:, 2] < cam.rmin + cam.ramp[2])}
    for side in list(sides) + ["far", "near"]:
        assert np.any(on[side]), "particle %d: no component on the %s ramp alone" % (i, side)
    assert np.count_nonzero(zero) >= 5 and np.count_nonzero(zero & (zh[:, 2] < 0)) >= 2, \
        "%d components at PD 0, %d of them behind the camera" % (np.count_nonzero(zero), np.count_nonzero(zero & (zh[:, 2] < 0)))
    pred = orc.predict(p, pose, f.z, (w, m, c))
    zpd = orc.detection_probability_m(p, f.z)
    xs = np.array([orc.measure_to_map(p, pose, zk) for zk in f.z])
    born = [k for b in pred[1][len(w):] for k in np.nonzero((xs == b).all(axis=1))[0]]
    assert any(0 < zpd[k] < p.pd for k in born), "no birth from a measurement in a ramp band (births from %r)" % (born,)
    return born


def assert_frame_bites(name, p, f):
    return [assert_bites(p, f, i, moved_sides(name)) for i in range(f.P)]


def on_cut_entries(p, f, i):
    """large_minw: the corrected entries of particle i that the frame plants ON MinWeight, by index into the corrected
    mixture — the misdetection copies of the ON_CUT components and of the birth from measurement Z_OUTSIDE (the copies come
    first, in the order of the predicted mixture)"""
    pred = orc.predict(p, f.poses[i], f.z, f.map(i))
    x = orc.measure_to_map(p, f.poses[i], f.z[Z_OUTSIDE])
    birth = [f.C + k for k, b in enumerate(pred[1][f.C:]) if (b == x).all()]
    return list(ON_CUT) + birth, len(birth)


def assert_frame_margins(p, f, z=None, what="", exempt=None):
    """rigid.assert_margins (gate-aware) on every particle; exempt: per particle, the corrected entries left out of the
    MinWeight margin. Returns the oracle's stages."""
    z = f.z if z is None else z
    return [rigid.assert_margins(p, f.poses[i], z, f.map(i), "%s particle %d" % (what, i), exempt=exempt[i] if exempt else ())
            for i in range(f.P)]


def assert_state_margins(p, st, z, what="", on_minw_exact=False):
    """the margins of a whole step's input state. on_minw_exact: corrected weights that EQUAL MinWeight bit for bit (what
    large_minw plants: 0.25 = (1 - 0) * 0.25 = (1 - 0.5) * 0.5, exact products) are left out of the MinWeight margin; one
    that is merely close still fails."""
    for i in range(st.P):
        ex = ()
        if on_minw_exact:
            pred = orc.predict(p, st.poses[i], z, st.map(i))
            ex = np.nonzero(orc.correct(p, st.poses[i], z, pred)[0] == p.min_weight)[0]
        rigid.assert_margins(p, st.poses[i], z, st.map(i), "%s particle %d" % (what, i), exempt=ex)


def gated_pairs(p, pose, z, means):
    """the (measurement, component) pairs inside the correction's gate"""
    g = gate2(p)
    out = set()
    for k, zk in enumerate(z):
        d2 = np.sum((means - measure_to_map(p, pose, zk)) ** 2, axis=1)
        out |= {(k, int(n)) for n in np.nonzero(d2 <= g)[0]}
    return out


def assert_set_bites(name, p, f, stages):
    """what SETS[name] must change on the frame f, stated on the reference (stages: the oracle's (predicted, corrected,
    pruned, alpha, set log-likelihood) per particle): a set that changes nothing tests nothing"""
    over = SETS[name]
    if "R" in over:
        pd_ = with_R(p, np.diag(np.diag(np.array(p.R).reshape(3, 3))))
        for i, (pred, cor, _, _, _) in enumerate(stages):
            dw = orc.correct(pd_, f.poses[i], f.z, pred)[0]
            assert len(dw) == len(cor[0])
            rel = np.abs(cor[0] - dw) / np.maximum(np.abs(dw), 1e-300)
            assert np.max(rel[dw > p.min_weight]) > 1e-3, "particle %d: R's correlations move no corrected weight" % i
    if "film" in over:
        d = params("correlated", f)   # (any set with the default camera)
        moved = sum(orc.detection_probability(p, f.poses[i], x) != orc.detection_probability(d, f.poses[i], x)
                    for i in range(f.P) for x in f.mean[i])
        assert moved >= 1, "no detection probability differs from the default camera's"
    if "max_quantity" in over and over["max_quantity"] < 600:
        for i, (_, cor, pr, _, _) in enumerate(stages):
            kept = np.count_nonzero(~(cor[0] < p.min_weight))
            assert kept > p.max_quantity, "particle %d: %d entries at or above MinWeight, the MaxQuantity cut is idle" % (i, kept)
            assert len(pr[0]) < p.max_quantity, "particle %d: no merge behind the cut" % i
    if name == "small_minw_wide":
        for i, (_, cor, pr, _, _) in enumerate(stages):
            assert len(pr[0]) >= 200, "particle %d: %d entries for the map estimate to rank" % (i, len(pr[0]))
    if "density_distance_threshold" in over:
        default = params("correlated", f)
        other = type(p).from_buffer_copy(p)
        other.gate_metric = PHD_GATE_SQUARED_EUCLIDEAN if p.gate_metric == PHD_GATE_EUCLIDEAN else PHD_GATE_EUCLIDEAN
        for i, (pred, _, _, _, _) in enumerate(stages):
            mine = gated_pairs(p, f.poses[i], f.z, pred[1])
            assert mine != gated_pairs(default, f.poses[i], f.z, pred[1]), "particle %d: the default gate's pairs" % i
            assert mine != gated_pairs(other, f.poses[i], f.z, pred[1]), "particle %d: the other metric's pairs at this radius" % i
    if name == "large_minw":
        for i, (pred, cor, pr, _, _) in enumerate(stages):
            ex, nbirth = on_cut_entries(p, f, i)
            assert nbirth >= 1, "particle %d: measurement %d is not born" % (i, Z_OUTSIDE)
            assert all(cor[0][j] == p.min_weight for j in ex), "particle %d: planted entries off MinWeight: %r" % (i, cor[0][ex])
            assert np.count_nonzero(pr[0] == p.min_weight) >= 2, "particle %d: the oracle does not keep the entries on MinWeight" % i
            x = orc.measure_to_map(p, f.poses[i], f.z[Z_OUTSIDE])
            assert any(wj == p.min_weight and (mj == x).all() for wj, mj in zip(pr[0], pr[1])), "particle %d: the birth on MinWeight is gone" % i


def stage_exempt(name, p, f):
    return [on_cut_entries(p, f, i)[0] for i in range(f.P)] if name == "large_minw" else None


def checked_frame(name, P, C, M, seed, **more):
    """(params, frame, the oracle's stages per particle) of a stage case, every precondition asserted"""
    p = params(name, P=P, M=M, C=C, **more)
    f = frame_for(p, P, C, M, seed, on_cut=(name == "large_minw"))
    assert_frame_bites(name, p, f)
    stages = assert_frame_margins(p, f, what=name, exempt=stage_exempt(name, p, f))
    assert_set_bites(name, p, f, stages)
    return p, f, stages


# ---- the table of stage and step cases -------------------------------------------------------------------------------
# (set, P, C, M): seed. A seed whose frame misses a precondition is replaced HERE, as a literal, never at run time.
STAGE_SHAPES = {name: [(4, 130, 32)] for name in PRM3D_SETS if name != "small_minw_wide"}
for _name in ("correlated", "camera", "filter", "all_of_it"):
    STAGE_SHAPES[_name].append((3, 300, 70))
STAGE_SHAPES["small_minw"] = [(4, 130, 32), (3, 60, 16)]
STAGE_SHAPES["small_minw_wide"] = [(3, 300, 64)]
STAGE_SEEDS = {}
STEP_SETS = ["correlated", "camera", "filter", "all_of_it", "euclid_small", "large_minw"]
STEP_SHAPES = [(16, 60, 20), (40, 130, 32)]
# filter at 40 particles: at MergeThreshold 1.5 the particles differ in WHICH pairs merge, and log alpha with it by 4: the
# first of the seeds from 322 whose first step does not resample (352; 322 - 351 all do)
STEP_SEEDS = {("filter", 40, 130, 32): 352}
# MinEffectiveParticle 0.6 must let a step pass without resampling: particles one odometry-noise step apart differ by
# tens in log alpha, N_eff / P of a few percent at every seed tried (1 - 24). A converged set (spread 0.005) weighs evenly in
# its first step; the host's motion then spreads it and the later steps resample.
STEP_SPREAD = {"filter": 0.005, "all_of_it": 0.005}


def stage_seed(name, shape):
    return STAGE_SEEDS.get((name,) + tuple(shape), 100 + 7 * PRM3D_SETS.index(name))


def step_seed(name, shape):
    return STEP_SEEDS.get((name,) + tuple(shape), 300 + 11 * PRM3D_SETS.index(name))


def step_inputs(p, f, seed, nsteps=3, spread=1.0):
    """per step: the host's pose motion (as tests/soak.py; the first step's times `spread`), the measurements perturbed by
    N(0, R) scaled by 0.2 s (the lone planted ones stay), u"""
    rng = np.random.default_rng([seed, 0x57e9])
    L = np.linalg.cholesky(np.array(p.R).reshape(3, 3))
    out = []
    for s in range(nsteps):
        z = f.z + (rng.normal(size=f.z.shape) @ L.T) * 0.2 * s
        z[NBAND:NPLANT_Z] = f.z[NBAND:NPLANT_Z]
        out.append((rng.normal(0, 2e-3, (f.P, 3)) * (spread if s == 0 else 1.0), z, float(rng.uniform(0.05, 0.95))))
    return out


def step_frame(name, shape):
    """(params, frame, seed) of a whole-step case, the planted layout asserted"""
    P, C, M = shape
    seed = step_seed(name, shape)
    p = params(name, P=P, C=C, M=M)
    f = frame_for(p, P, C, M, seed, on_cut=(name == "large_minw"), spread=STEP_SPREAD.get(name, 1.0))
    assert_frame_bites(name, p, f)
    return p, f, seed


def oracle_steps(name, p, f, seed, threads=8):
    """the oracle's run of a step case, margins asserted on every step's input state: per step (poses, z, u, state after,
    best, src, res)"""
    from oracle_parity import oracle_state
    st = oracle_state(f, max(p.max_quantity, f.C))
    out = []
    for s, (dpose, z, u) in enumerate(step_inputs(p, f, seed, spread=STEP_SPREAD.get(name, 1.0))):
        st.poses[:, :3] += dpose
        what = "%s step %d" % (name, s)
        assert_state_margins(p, st, z, what, on_minw_exact=(name == "large_minw"))
        prior = st.weights.copy()
        poses = st.poses.copy()
        best, src, res, alpha = orc.slam_update(p, st, z, u=u, threads=threads)
        rigid.assert_neff_margin(p, prior, alpha, what)
        out.append((poses, z, u, st.copy(), best, src, res))
    return out


def pd_one_case(P=3, C=40, M=12, seed=500):
    """(params, frame, the oracle's stages per particle) at PD = 1: log(1 - PD) = -inf for every landmark in full view.
    The margins of a stage case but for the finiteness of alpha: here the class of every particle (finite, or -inf and 0)
    is what the device must reproduce."""
    p = params("correlated", P=P, C=C, M=M, pd=1.0)
    f = frame_for(p, P, C, M, seed)
    assert_frame_bites("correlated", p, f)
    stages = []
    for i in range(P):
        pose, mix = f.poses[i], f.map(i)
        assert rigid.off(rigid.explored_density(p, pose, f.z, mix), p.exploration_threshold, 1e-6)
        pred = orc.predict(p, pose, f.z, mix)
        rigid.assert_gate_margins(p, pose, f.z, mix, pred, "pd 1 particle %d" % i)
        cor = orc.correct(p, pose, f.z, pred)
        assert rigid.off(cor[0], p.min_weight, 1e-6)
        pr = orc.prune(p, cor)
        a, sll = orc.weight_alpha(p, pose, f.z, pred, pr)
        stages.append((pred, cor, pr, a, sll))
    return p, f, stages
