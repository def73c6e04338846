"""Shared by tests/test_ascent_abi.py and tests/test_gpu_ascent.py: a counting proxy around a navigator's batch evaluations,
which tells how many iterations the host-driven ascent ran per estimate, and the numpy statement of one control step of the
ascent (the clip, the 16 halved steps, the do-while of LoopyPHDNavigator.cs:943-951)."""
import numpy as np

from monorfs_amd.navigator import pose3d_add


class CountingNav:
    """Forwards QuasiSetLogLikelihood[Gradient] to `nav` and keeps the pose batches. loopy.LogLikeGradientAscent's gradient
    batches after the first hold the last tried poses of the estimates still active, in order; each is one of the 16
    candidates of that estimate in the value batch before (or, for the first, its starting pose), bit for bit: that is how
    iterations() tells which estimates a batch held."""

    def __init__(self, nav):
        self.nav, self.params = nav, nav.params
        self.batches = []   # ("g" | "v", poses[k][7])

    def QuasiSetLogLikelihood(self, measurements, landmarks, poses):
        self.batches.append(("v", np.array(poses, float).reshape(-1, 7)))
        return self.nav.QuasiSetLogLikelihood(measurements, landmarks, poses)

    def QuasiSetLogLikelihoodGradient(self, measurements, landmarks, poses, average_mode=0):
        self.batches.append(("g", np.array(poses, float).reshape(-1, 7)))
        return self.nav.QuasiSetLogLikelihoodGradient(measurements, landmarks, poses, average_mode)

    def iterations(self):
        """per estimate: the gradient batches of the loop (all but the first) it was part of; an estimate's line search follows
        each of them"""
        assert self.batches and self.batches[0][0] == "g"
        n = len(self.batches[0][1])
        counts = np.zeros(n, np.int32)
        active = list(range(n))
        tried = {a: [self.batches[0][1][a].tobytes()] for a in active}
        for kind, poses in self.batches[1:]:
            if kind == "g":
                now, u = [], 0
                for row in poses:
                    while row.tobytes() not in tried[active[u]]:
                        u += 1
                    now.append(active[u])
                    u += 1
                active = now
                counts[active] += 1
            else:
                assert len(poses) == 16 * len(active)
                tried = {a: [r.tobytes() for r in poses[16 * u:16 * u + 16]] for u, a in enumerate(active)}
        return counts


def control_reference(pose6, loglike, grad, values, lin):
    """One iteration of loopy.LogLikeGradientAscent between its two evaluations, per estimate, with `values[n][16]` standing for
    the value batch: returns cand6[n][16][6], cand7[n][16][7], chosen[n], newpose6, newloglike, nextpose7[n][7], active[n]."""
    pose6, grad, values = np.array(pose6, float).reshape(-1, 6), np.asarray(grad, float).reshape(-1, 6), np.asarray(values, float).reshape(-1, 16)
    loglike = np.array(loglike, float).reshape(-1)
    n = len(pose6)
    cand6, cand7 = np.empty((n, 16, 6)), np.empty((n, 16, 7))
    chosen, active, nextpose7 = np.zeros(n, np.int32), np.zeros(n, np.int32), np.empty((n, 7))
    for a in range(n):
        g = grad[a]
        size = np.linalg.norm(g)
        if size > 10.0:
            g = g * (10.0 / size)
        multiplier = 1e-2
        for c in range(16):
            cand6[a, c] = pose6[a] + multiplier * g
            cand7[a, c] = pose3d_add(lin, cand6[a, c])
            multiplier /= 2.0
        c = 0
        while True:
            v = values[a, c]
            c += 1
            if not (v < loglike[a] and c < 16):
                break
        chosen[a] = c - 1
        nextpose7[a] = cand7[a, c - 1]
        prev = loglike[a]
        if v > loglike[a]:
            pose6[a] = cand6[a, c - 1]
            loglike[a] = v
        active[a] = 1 if loglike[a] - prev > 1e-3 else 0
    return cand6, cand7, chosen, pose6, loglike, nextpose7, active
