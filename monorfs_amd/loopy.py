"""Host mirror of the pose searches of the reference's smoother: the static functions of
LoopyPHDNavigator that evaluate QuasiSetLogLikelihood and its gradient for candidate poses against one map estimate
and one measurement set (LoopyPHDNavigator.cs:718-1021), Filter / FilterMissing (:713-762), and LeaveOneOutMaps: the
FilterMissing of every frame of UpdateMessagesFromMap (:511-552) from one pass of held steps.

Every evaluation goes to the device through PHDNavigator.QuasiSetLogLikelihood / QuasiSetLogLikelihoodGradient
(phd_quasi_set_loglik, phd_quasi_set_loglik_grad) as a BATCH: the 16 step sizes of a line search at once, all the
starting guesses of GuidedFitMixture side by side, the 12 gradient evaluations of the covariance fit together. The
results per pose are those of the reference's one-at-a-time loops, evaluations are independent of each other.

Not pinned (third-party code outside the reference tree, Accord.Math 3.0.2): EigenvalueDecomposition of the
finite-difference Hessian, PseudoInverse and PseudoDeterminant of 6 x 6 matrices; numpy stands in, see
LogLikeFitCovariance."""
import math

import numpy as np

from .navigator import pose3d_add

OdoSize = 6
GradientAscentRate = 1e-2   # Config.cs:94
GradientClip = 10.0         # Config.cs:95


# ---------------------------------------------------------------------------------------------- quaternions / Pose3D
def _qmul(a, b):   # Quaternion.cs:295-301
    return np.array([a[0] * b[0] - (a[1] * b[1] + a[2] * b[2] + a[3] * b[3]),
                     a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3],
                     a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]])


def _qconj(q):
    return np.array([q[0], -q[1], -q[2], -q[3]])


def _qmatrix(q):   # Quaternion.ToMatrix, Quaternion.cs:327-342
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _qlog(q):   # Quaternion.Log, Quaternion.cs:204-218
    q = np.asarray(q, float) / np.linalg.norm(q)
    phi = math.acos(min(1.0, max(-1.0, q[0])))
    mag = np.linalg.norm(q[1:])
    if mag < 1e-12:
        return np.zeros(3)
    return phi * (q[1:] / mag)


def vector_rotator(a, b):
    """Quaternion.VectorRotator (Quaternion.cs:281-284): the rotation taking unit vector a into unit vector b"""
    q = np.concatenate([[1 + np.dot(a, b)], np.cross(a, b)])
    return q / np.linalg.norm(q)


def pose3d_subtract(pose7, origin7):
    """Pose3D.Subtract (Pose3D.cs:296-308): the linear vector that takes `origin` into `pose`"""
    pose7, origin7 = np.asarray(pose7, float), np.asarray(origin7, float)
    qo = origin7[3:]
    dq = _qmul(_qconj(qo), pose7[3:])
    dxg = pose7[:3] - origin7[:3]
    dx = _qmul(_qmul(_qconj(qo), np.concatenate([[0.0], dxg])), qo)
    return np.concatenate([dx[1:], 2 * _qlog(dq)])   # dq.ToLinear() = dq.Subtract(Identity) = 2 Log(dq), Quaternion.cs:176-179


def fit_to_measurement(params, pose0, measurement, landmark):
    """PRM3DMeasurer.FitToMeasurement (PRM3DMeasurer.cs:224-244): the pose near pose0 from which `landmark` would be
    measured as `measurement`"""
    pose0 = np.asarray(pose0, float)
    focal = params.measurer[0]
    q0 = pose0[3:]
    diff = np.asarray(landmark, float) - pose0[:3]
    landmarklocal = _qmatrix(_qconj(q0)) @ diff
    px, py, rng = measurement
    ml = np.zeros(3)
    ml[2] = rng / math.sqrt(1 + (px * px + py * py) / (focal * focal))
    ml[0] = px * ml[2] / focal
    ml[1] = py * ml[2] / focal
    align = vector_rotator(landmarklocal / np.linalg.norm(landmarklocal), ml / np.linalg.norm(ml))
    rotation = _qmul(_qconj(align), q0)
    location = np.asarray(landmark, float) - _qmatrix(rotation) @ ml
    return np.concatenate([location, rotation / np.linalg.norm(rotation)])   # new Pose3D normalises (Pose3D.cs:157-161)


def best_map_estimate(model):
    """Map.BestMapEstimate (Map.cs:119-142): (int) ExpectedSize picks from the weight-sorted list, each pick re-entered
    with its weight less one; stable order on ties (the canonical order of the device path). Returns the means [J][3]."""
    w, m, _ = model
    w = np.asarray(w, float)
    size = int(np.sum(w))
    lst = sorted(((w[i], i) for i in range(len(w))), key=lambda e: -e[0])
    picks = []
    for i in range(size):
        wi, src = lst[i]
        picks.append(src)
        lst.append((wi - 1, src))
        lst.sort(key=lambda e: -e[0])
    return np.asarray(m, float).reshape(-1, 3)[picks].reshape(-1, 3)


# ---------------------------------------------------------------------------------------------- batched evaluation
def _batches(n, cap):
    for s in range(0, n, cap):
        yield s, min(n, s + cap)


def _values(nav, measurements, landmarks, poses7):
    poses7 = np.asarray(poses7, float).reshape(-1, 7)
    out = np.empty(len(poses7))
    for s, e in _batches(len(poses7), nav.params.max_particles):
        out[s:e] = nav.QuasiSetLogLikelihood(measurements, landmarks, poses7[s:e])
    return out


def _values_gradients(nav, measurements, landmarks, poses7, average_mode):
    poses7 = np.asarray(poses7, float).reshape(-1, 7)
    out, grad = np.empty(len(poses7)), np.empty((len(poses7), 6))
    for s, e in _batches(len(poses7), nav.params.max_particles):
        out[s:e], grad[s:e] = nav.QuasiSetLogLikelihoodGradient(measurements, landmarks, poses7[s:e], average_mode)
    return out, grad


ResidentIterationBound = 1000   # resident=True without max_iterations: what bounds the device call (reaching it raises)


def _resident_ascent(nav, initial, measurements, landmarks, linearpoint, average_mode, max_iterations, hessians=False):
    """the whole search as device calls (PHDNavigator.QuasiAscent chunks by max_particles // 16). Without max_iterations an
    estimate still climbing at ResidentIterationBound is an error: the reference's loop has no bound to truncate at."""
    bound = ResidentIterationBound if max_iterations is None else int(max_iterations)
    out = nav.QuasiAscent(initial, measurements, landmarks, linearpoint, average_mode, max_iterations=bound, hessians=hessians)
    if out[3] and max_iterations is None:
        raise RuntimeError("LogLikeGradientAscent(resident=True): still climbing after %d iterations" % bound)
    return out


def LogLikeGradientAscent(nav, initial, measurements, landmarks, linearpoint, average_mode=0, resident=False, max_iterations=None):
    """≙ LoopyPHDNavigator.LogLikeGradientAscent (:916-965) for one initial estimate [6] or several [n][6] run side by
    side. Returns (pose, loglike) or (poses[n][6], loglikes[n]).

    Per estimate, exactly the reference's loop: the analytic gradient at the LAST TRIED pose (`nextvehicle`, :933-934 —
    after a rejected step that is not the current one), clipped to GradientClip, step GradientAscentRate halved up to 16
    times until the value does not decrease (:943-951), until an iteration gains no more than 1e-3. The 16 candidate
    steps of an iteration are evaluated as one device batch and the first acceptable one is taken.

    resident=True: the same loop as ONE device call per max_particles // 16 estimates (nav.QuasiAscent, phd_quasi_ascent);
    the host sees neither gradients nor candidates. max_iterations: stop every estimate after that many iterations (the
    reference has no bound; None: none here, ResidentIterationBound on the device)."""
    initial = np.asarray(initial, float)
    single = initial.ndim == 1
    if resident:
        pose, loglike = _resident_ascent(nav, initial.reshape(-1, OdoSize), measurements, landmarks, linearpoint, average_mode, max_iterations)[:2]
        return (pose[0], loglike[0]) if single else (pose, loglike)
    pose = initial.reshape(-1, OdoSize).copy()
    n = len(pose)
    lin = np.asarray(linearpoint, float)
    nextpose7 = np.array([pose3d_add(lin, pose[a]) for a in range(n)])
    loglike, _ = _values_gradients(nav, measurements, landmarks, nextpose7, average_mode)   # :928-929
    prevvalue = np.full(n, -np.inf)
    active = [a for a in range(n) if loglike[a] - prevvalue[a] > 1e-3]
    iteration = 0
    while active and (max_iterations is None or iteration < max_iterations):
        iteration += 1
        _, grad = _values_gradients(nav, measurements, landmarks, nextpose7[active], average_mode)   # :933-934
        cand6 = np.empty((len(active), 16, OdoSize))
        for u, a in enumerate(active):
            g = grad[u]
            size = np.linalg.norm(g)
            if size > GradientClip:
                g = g * (GradientClip / size)
            multiplier = GradientAscentRate
            for c in range(16):
                cand6[u, c] = pose[a] + multiplier * g
                multiplier /= 2.0
        cand7 = np.array([[pose3d_add(lin, cand6[u, c]) for c in range(16)] for u in range(len(active))])
        vals = _values(nav, measurements, landmarks, cand7.reshape(-1, 7)).reshape(len(active), 16)
        still = []
        for u, a in enumerate(active):
            c = 0
            while True:   # do { ... counter++ } while (nextloglike < loglike && counter < 16)
                nextloglike = vals[u, c]
                c += 1
                if not (nextloglike < loglike[a] and c < 16):
                    break
            nextpose7[a] = cand7[u, c - 1]
            prevvalue[a] = loglike[a]
            if nextloglike > loglike[a]:
                pose[a] = cand6[u, c - 1]
                loglike[a] = nextloglike
            if loglike[a] - prevvalue[a] > 1e-3:
                still.append(a)
        active = still
    return (pose[0], loglike[0]) if single else (pose, loglike)


def LogLikeFitCovariance(nav, pose, measurements, landmarks, linearpoint, average_mode=0):
    """≙ LoopyPHDNavigator.LogLikeFitCovariance (:976-1021): Hessian rows by central differences (eps = 1e-5) of the
    analytic gradient — 12 gradient evaluations, one device batch —, NaN -> zero matrix, positive eigenvalues clipped
    to zero, covariance = pinv(-Hessian).

    The reference decomposes the (not exactly symmetric) finite-difference Hessian with Accord's general
    EigenvalueDecomposition and recombines V D V'; that code is outside the tree. Here the symmetric part is decomposed
    (numpy.linalg.eigh), which is the same thing whenever the Hessian is symmetric. Unpinned, as the module header says."""
    pose = np.asarray(pose, float).reshape(OdoSize)
    lin = np.asarray(linearpoint, float)
    eps = 1e-5
    cand = np.empty((OdoSize, 2, 7))
    for i in range(OdoSize):
        for s, sign in enumerate((1.0, -1.0)):
            d = pose.copy()
            d[i] += sign * eps
            cand[i, s] = pose3d_add(lin, d)
    _, g = _values_gradients(nav, measurements, landmarks, cand.reshape(-1, 7), average_mode)
    g = g.reshape(OdoSize, 2, OdoSize)
    return HessianToCovariance((g[:, 0] - g[:, 1]) / (2 * eps))


def HessianToCovariance(hessian):
    """The tail of LogLikeFitCovariance (:1003-1021) from the raw finite-difference rows on: NaN -> zero matrix, positive
    eigenvalues of the symmetric part clipped to zero, pinv(-Hessian). Shared by the host-driven and the resident path."""
    hessian = np.asarray(hessian, float).reshape(OdoSize, OdoSize)
    if np.isnan(hessian).any():
        hessian = np.zeros((OdoSize, OdoSize))
    vals, vecs = np.linalg.eigh(0.5 * (hessian + hessian.T))
    hessian = vecs @ np.diag(np.minimum(0.0, vals)) @ vecs.T
    return np.linalg.pinv(-hessian)


def FitGaussian(nav, pose0, measurements, landmarks, linearpoint, average_mode=0, resident=False, max_iterations=None):
    """≙ LoopyPHDNavigator.FitGaussian (:863-869): (mean, covariance) of weight 1. resident=True: the ascent and the Hessian
    rows at its maximum come from one device call (nav.QuasiAscent)."""
    if resident:
        pose, _, _, _, hess = _resident_ascent(nav, np.asarray(pose0, float).reshape(1, OdoSize), measurements, landmarks, linearpoint, average_mode,
                                               max_iterations, hessians=True)
        return pose[0], HessianToCovariance(hess[0])
    maxpose, _ = LogLikeGradientAscent(nav, pose0, measurements, landmarks, linearpoint, average_mode, max_iterations=max_iterations)
    return maxpose, LogLikeFitCovariance(nav, maxpose, measurements, landmarks, linearpoint, average_mode)


def _pseudo_determinant(m):
    sv = np.linalg.svd(m, compute_uv=False)
    tol = max(m.shape) * np.finfo(float).eps * (sv[0] if len(sv) else 0.0)
    nz = sv[sv > tol]
    return float(np.prod(nz)) if len(nz) else 0.0


def GuidedFitMixture(nav, pose0, measurements, model, linearpoint, average_mode=0, resident=False, max_iterations=None):
    """≙ LoopyPHDNavigator.GuidedFitMixture (:777-852). `model` = (w, mean, cov) of the map. Returns
    (emptyspace, [(weight, mean[6], cov[6][6]), ...]).

    As in the reference: guesses = pose0 plus, for every (landmark of the map estimate, measurement) pair, the pose
    that explains the pair if it lies within 0.5 of the initial pose (:790-798); a guess worse than a pose far from
    everything is dropped (:821-823); each remaining guess climbs (all of them side by side here); a maximum within
    Mahalanobis 0.1 of an earlier component is dropped (:827-837); the covariance is fitted at `maxpose`, which the
    reference never updates from pose0 (:800, :839), so it is computed once. resident / max_iterations: as for
    LogLikeGradientAscent, for the climb of the guesses."""
    pose0 = np.asarray(pose0, float).reshape(OdoSize)
    lin = np.asarray(linearpoint, float)
    z = np.asarray(measurements, float).reshape(-1, 3)
    initpose = pose3d_add(lin, pose0)
    jmap = best_map_estimate(model)
    guesses = [pose0]
    for landmark in jmap:
        for measurement in z:
            guess = fit_to_measurement(nav.params, initpose, measurement, landmark)
            d = pose3d_subtract(guess, initpose)
            if float(np.dot(d, d)) < 0.5 * 0.5:
                guesses.append(pose3d_subtract(guess, lin))
    identity = np.array([0, 0, 0, 1.0, 0, 0, 0])
    infpose = pose3d_add(identity, np.full(OdoSize, 1e5))
    first = _values(nav, z, jmap, np.array([infpose] + [pose3d_add(lin, g) for g in guesses]))
    emptyspace = first[0]
    climbing = [g for g, v in zip(guesses, first[1:]) if not (v - emptyspace < 0)]
    if not climbing:
        return emptyspace, []
    poses, values = LogLikeGradientAscent(nav, np.array(climbing), z, jmap, lin, average_mode, resident, max_iterations)
    return emptyspace, _mixture_of(poses, values, lambda: LogLikeFitCovariance(nav, pose0, z, jmap, lin, average_mode))


def _mixture_of(poses, values, localcov):
    """the tail of GuidedFitMixture (:825-850): maxima in order, one within Mahalanobis 0.1 of an earlier component dropped,
    every component with the covariance fitted at pose0 (`localcov`: a callable, evaluated on first need)"""
    components = []
    cov = None
    for localpose, localmax in zip(poses, values):
        counted = False
        for _, mean, c in components:
            diff = mean - localpose
            if math.sqrt(max(0.0, diff @ np.linalg.pinv(c) @ diff)) < 0.1:
                counted = True
                break
        if counted:
            continue
        if cov is None:
            cov = localcov()
        # Math.Pow(2 pi, -localpose.Length / 2): integer division, exponent -3
        with np.errstate(divide="ignore"):
            logmultiplier = math.log((2 * math.pi) ** (-(OdoSize // 2))) - 0.5 * np.log(_pseudo_determinant(cov))
        components.append((math.exp(localmax - logmultiplier), localpose, cov))
    return components


def _far_pose():
    """the pose far from everything (:808)"""
    return pose3d_add(np.array([0, 0, 0, 1.0, 0, 0, 0]), np.full(OdoSize, 1e5))


def _problems_of(pose0s, measurement_sets, models, linearpoints):
    """frame i as a problem (map estimate, measurements, linearisation pose) of the multi calls, and its initial linear pose"""
    problems = [(best_map_estimate(models[i]), np.asarray(measurement_sets[i], float).reshape(-1, 3), np.asarray(linearpoints[i], float))
                for i in range(len(pose0s))]
    return problems, [np.asarray(p, float).reshape(OdoSize) for p in pose0s]


def HostGuessLists(params, problems, pose0s, radius=0.5):
    """The guess loop of GuidedFitMixture (:789-797) per frame, on the host alone: (guesses, pairs) — frame i's guesses are pose0,
    then every (landmark, measurement) pair whose fitted pose lies within `radius` of the initial pose, landmark-major;
    pairs[i][e] = (landmark, measurement) of guess e, (-1, -1) for pose0."""
    guesses, pairs = [], []
    for (jmap, z, lin), pose0 in zip(problems, pose0s):
        initpose = pose3d_add(lin, pose0)
        mine, who = [pose0], [(-1, -1)]
        for j, landmark in enumerate(jmap):
            for m, measurement in enumerate(z):
                guess = fit_to_measurement(params, initpose, measurement, landmark)
                d = pose3d_subtract(guess, initpose)
                if float(np.dot(d, d)) < radius * radius:
                    mine.append(pose3d_subtract(guess, lin))
                    who.append((j, m))
        guesses.append(mine)
        pairs.append(who)
    return guesses, pairs


def HostGuesses(nav, problems, pose0s, radius=0.5):
    """The guess stage of GuidedFitMixtures on the host (:789-823): HostGuessLists, then the first values of every guess and the
    value of the pose far from everything, those of all frames from ONE device call (QuasiSetLogLikelihoodMulti).
    Returns (guesses, firsts, empties, pairs): lists per frame."""
    infpose = _far_pose()
    guesses, pairs = HostGuessLists(nav.params, problems, pose0s, radius)
    poses7, which, at = [], [], []
    for i, ((_, _, lin), mine) in enumerate(zip(problems, guesses)):
        at.append(len(poses7))
        poses7 += [infpose] + [pose3d_add(lin, g) for g in mine]
        which += [i] * (1 + len(mine))
    first = nav.QuasiSetLogLikelihoodMulti(problems, np.array(poses7).reshape(-1, 7), which) if problems else np.zeros(0)
    return guesses, [first[a + 1:a + 1 + len(g)] for a, g in zip(at, guesses)], [first[a] for a in at], pairs


def DeviceGuesses(nav, problems, pose0s, radius=0.5):
    """HostGuesses from the device: the guesses, their first values and the far pose's values of all frames from the ONE call
    nav.QuasiGuessesMulti (phd_quasi_guesses_multi). The same lists in the same order; a guess agrees with the host's to rounding."""
    if not problems:
        return [], [], [], []
    off, pairs, g6, _, values, empties = nav.QuasiGuessesMulti(problems, pose0s, radius)
    cut = lambda a: [a[off[i]:off[i + 1]] for i in range(len(problems))]
    return [list(g) for g in cut(g6)], cut(values), list(empties), [[tuple(int(v) for v in p) for p in f] for f in cut(pairs)]


def FitMixturesFromGuesses(nav, problems, pose0s, guesses, firsts, empties, average_mode=0, max_iterations=None):
    """The stage of GuidedFitMixtures behind the guesses (:821-850), for all frames: a guess worse than the far pose is dropped,
    the others climb in ONE device call (QuasiAscentMulti), the 12 Hessian poses at pose0 of every frame that kept a guess are
    ONE more (QuasiSetLogLikelihoodGradientMulti); the dedupe and the weights stay per frame on the host. guesses[i], firsts[i],
    empties[i]: frame i's guess list, the first values of its guesses, the far pose's value (HostGuesses / DeviceGuesses)."""
    T = len(problems)
    climbing, owner = [], []
    for i in range(T):
        for g, v in zip(guesses[i], firsts[i]):
            if not (v - empties[i] < 0):
                climbing.append(g)
                owner.append(i)
    results = [(empties[i], []) for i in range(T)]
    if not climbing:
        return results
    bound = ResidentIterationBound if max_iterations is None else int(max_iterations)
    poses, values, _, capped = nav.QuasiAscentMulti(problems, np.array(climbing), owner, average_mode, max_iterations=bound)
    if capped and max_iterations is None:
        raise RuntimeError("GuidedFitMixtures: still climbing after %d iterations" % bound)
    kept = sorted(set(owner))
    eps = 1e-5
    hposes, hwhich = [], []
    for i in kept:   # the 12 poses of LogLikeFitCovariance at pose0 (which the reference never updates, :800, :839)
        pose0, lin = pose0s[i], problems[i][2]
        for t in range(OdoSize):
            for sign in (1.0, -1.0):
                d = pose0.copy()
                d[t] += sign * eps
                hposes.append(pose3d_add(lin, d))
                hwhich.append(i)
    _, g = nav.QuasiSetLogLikelihoodGradientMulti(problems, np.array(hposes), hwhich, average_mode)
    g = g.reshape(len(kept), OdoSize, 2, OdoSize)
    owner = np.asarray(owner)
    for k, i in enumerate(kept):
        mine = np.nonzero(owner == i)[0]
        cov = HessianToCovariance((g[k, :, 0] - g[k, :, 1]) / (2 * eps))
        results[i] = (empties[i], _mixture_of(poses[mine], values[mine], lambda cov=cov: cov))
    return results


def GuidedFitMixturesRouted(nav, pose0s, measurement_sets, models, linearpoints, average_mode=0, max_iterations=None, device_guesses=False):
    """GuidedFitMixture(..., resident=True) for many frames at once (≙ the Parallel.For of UpdateMessagesFromMap, :525-551):
    frame i has the initial linear pose pose0s[i], the measurements measurement_sets[i], the map models[i] = (w, mean, cov) and
    the linearisation pose linearpoints[i]. Returns the list of (emptyspace, components).

    Two stages. The guess stage makes every frame's guesses and their first values: on the host with one batch call
    (HostGuesses; frame i's result is then exactly GuidedFitMixture's with resident=True), or with device_guesses=True as the
    one call nav.QuasiGuessesMulti (DeviceGuesses) — the same lists, each guess to rounding. FitMixturesFromGuesses does the
    rest with two more device calls. A `nav` without the multi methods takes the per-frame calls: that fallback states what the
    calls mean."""
    T = len(pose0s)
    if not hasattr(nav, "QuasiAscentMulti"):
        if device_guesses:
            raise ValueError("device_guesses=True needs a navigator with QuasiGuessesMulti")
        resident = hasattr(nav, "QuasiAscent")   # (the oracle stub has the batch calls alone: the host drives its loop)
        return [GuidedFitMixture(nav, pose0s[i], measurement_sets[i], models[i], linearpoints[i], average_mode, resident, max_iterations) for i in range(T)]
    problems, starts = _problems_of(pose0s, measurement_sets, models, linearpoints)
    guesses, firsts, empties, _ = (DeviceGuesses if device_guesses else HostGuesses)(nav, problems, starts)
    return FitMixturesFromGuesses(nav, problems, starts, guesses, firsts, empties, average_mode, max_iterations)


def GuidedFitMixtures(nav, pose0s, measurement_sets, models, linearpoints, average_mode=0, max_iterations=None):
    """GuidedFitMixturesRouted with the guesses of every frame made on the host: frame i's result is exactly what
    GuidedFitMixture(nav, pose0s[i], measurement_sets[i], models[i], linearpoints[i], average_mode, True, max_iterations) gives.
    THREE device calls serve all frames (PHDNavigator's QuasiSetLogLikelihoodMulti, QuasiAscentMulti,
    QuasiSetLogLikelihoodGradientMulti)."""
    return GuidedFitMixturesRouted(nav, pose0s, measurement_sets, models, linearpoints, average_mode, max_iterations, False)


def MapMessageMixturesRouted(nav, trajectory, factors, pose0s, linearpoints, to=None, average_mode=0, device_guesses=False):
    """The device part of LoopyPHDNavigator.UpdateMessagesFromMap (:511-552): LeaveOneOutMaps, then GuidedFitMixturesRouted over
    the frames < to that have measurements against the map each of them was left out of. Returns one (emptyspace, components)
    per frame; a frame without measurements gives (0.0, []) (:527-530). The temperature term and the fusions stay with the
    caller. pose0s[i] / linearpoints[i]: the initial linear pose and the linearisation pose of frame i; device_guesses: the
    guess stage as one device call."""
    to = len(trajectory) if to is None else min(len(trajectory), to)
    maps, _ = LeaveOneOutMaps(nav, trajectory, factors, to=to)
    seen = [i for i in range(to) if len(np.asarray(factors[i][1], float).reshape(-1, 3)) > 0]
    fits = GuidedFitMixturesRouted(nav, [pose0s[i] for i in seen], [factors[i][1] for i in seen], [maps[i] for i in seen],
                                   [linearpoints[i] for i in seen], average_mode, None, device_guesses)
    out = [(0.0, []) for _ in range(to)]
    for i, fit in zip(seen, fits):
        out[i] = fit
    return out


def MapMessageMixtures(nav, trajectory, factors, pose0s, linearpoints, to=None, average_mode=0):
    """MapMessageMixturesRouted with the guesses made on the host"""
    return MapMessageMixturesRouted(nav, trajectory, factors, pose0s, linearpoints, to, average_mode, False)


# ---------------------------------------------------------------------------------------------- Filter / FilterMissing
def FilterMissing(nav, trajectory, factors, index, to):
    """≙ LoopyPHDNavigator.FilterMissing (:729-762): a fresh one-particle, mapping-only PHD filter run over the poses
    trajectory[i] = (time, pose7) with the measurement sets factors[i] = (time, [[px, py, range], ...]), frame `index`
    left out, frames from `to` on ignored. Returns BestMapModel (w, mean, cov).

    `nav` is reset (one particle, empty map, mapping only): ≙ InnerFilter = new PHDNavigator(RefVehicle, 1, true)."""
    to = min(len(trajectory), to)
    index = to if index < 0 else min(to, index)
    empty = (np.zeros(0), np.zeros((0, 3)), np.zeros((0, 3, 3)))
    nav.OnlyMapping = True
    nav.reset(np.asarray(trajectory[0][1], float) if len(trajectory) else np.array([0, 0, 0, 1.0, 0, 0, 0]), empty, 1)
    for i in list(range(0, index)) + list(range(index + 1, to)):
        nav.set_poses(np.asarray(trajectory[i][1], float).reshape(1, 7))   # InnerFilter.BestEstimate.Pose = trajectory[i].Item2
        nav.SlamUpdate(trajectory[i][0], np.asarray(factors[i][1], float).reshape(-1, 3))
    return nav.BestMapModel


def Filter(nav, trajectory, factors):
    """≙ LoopyPHDNavigator.Filter (:718-721)"""
    return FilterMissing(nav, trajectory, factors, len(trajectory), len(trajectory))


def LeaveOneOutMaps(nav, trajectory, factors, indices=None, to=None):
    """The maps FilterMissing gives for each of `indices`, and Filter's over the frames < to, from ONE pass over the frames:
    returns (maps, full) with maps[j] bit for bit FilterMissing(nav, trajectory, factors, indices[j], to) and `full` the map
    with nothing left out (≙ the loop of LoopyPHDNavigator.UpdateMessagesFromMap, :511-552, around FilterMissing :729-762).

    The leave-one-out filters see the same poses and measurement sets and differ in the one frame each skips, and the
    particles of a mapping-only step are independent: they are the particles of one handle stepped together, the particle
    that leaves frame k out held through step k (PHDNavigator.StepHold, phd_step_hold_async); one more particle is never
    held. `nav` is reset (mapping only, empty maps). Every frame is posted without waiting — poses, measurements (an empty
    set is a step like any other), the held step —, one sync ends the pass and one download reads the maps.

    indices: default every frame < to; an index < 0 or >= to leaves nothing out (:733-734), duplicates are allowed. More
    distinct indices than max_particles - 1 run as several passes; `full` is the first pass's."""
    to = len(trajectory) if to is None else min(len(trajectory), to)
    indices = list(range(to)) if indices is None else [int(i) for i in indices]
    distinct = sorted({i for i in indices if 0 <= i < to})
    room = nav.params.max_particles - 1
    if distinct and room < 1:
        raise ValueError("LeaveOneOutMaps: a handle of at least two particles (one per left-out frame and one for the full map)")
    empty = (np.zeros(0), np.zeros((0, 3)), np.zeros((0, 3, 3)))
    pose0 = np.asarray(trajectory[0][1], float) if len(trajectory) else np.array([0, 0, 0, 1.0, 0, 0, 0])
    nav.OnlyMapping = True
    result, full = {}, None
    for s in range(0, max(len(distinct), 1), max(room, 1)):
        chunk = distinct[s:s + room]
        slot = {index: j for j, index in enumerate(chunk)}
        count = len(chunk) + 1                    # the last particle is never held: the full map
        nav.reset(pose0, empty, count)
        for k in range(to):
            nav.set_poses(np.tile(np.asarray(trajectory[k][1], float).reshape(1, 7), (count, 1)))
            nav.set_measurements(np.asarray(factors[k][1], float).reshape(-1, 3))
            nav.StepHold(slot.get(k, -1))
        nav.sync()
        _, counts, _, _ = nav.download_state(0)
        planes, counts, _, _ = nav.download_state(max(int(counts.max()), 1))
        models = [_model_of(planes, counts, j) for j in range(count)]
        result.update({index: models[j] for index, j in slot.items()})
        if full is None:
            full = models[count - 1]
    return [result.get(i, full) if 0 <= i < to else full for i in indices], full


def _model_of(planes, counts, particle):
    """(w, mean, cov) of one particle of a downloaded state: the device's records (covariance: upper triangle) as phd_map
    hands them out"""
    n = int(counts[particle])
    r = planes[:, particle, :n]
    cov = np.empty((n, 3, 3))
    for f, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        cov[:, a, b] = cov[:, b, a] = r[4 + f]
    return r[0].copy(), np.ascontiguousarray(r[1:4].T), cov
