"""Whole steps of a handle against the CPU oracle (tests/orc.py), every particle at once: the device state is read in bulk
(phd_download_state_soa) and compared with the oracle's flat state with the tolerances of
test_gpu_round2.test_config_A_full_size_step — resampling flag, sources and BestParticle exact, particle weights within rtol
1e-6, every map within 1e-7 (weights, means, upper-triangle covariances), OSPA of the best map estimate below 1e-4."""
import numpy as np

import orc

# the planes of phd_download_state_soa: w, mean xyz, cov xx xy xz yy yz zz
_UT = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]


def oracle_state(f, cap):
    """the oracle's copy of a synth.Frame's particle set (poses, maps, weights)"""
    st = orc.State(f.P, cap)
    st.poses[:] = f.poses
    st.w[:, :f.C], st.mean[:, :f.C], st.cov[:, :f.C], st.n[:] = f.w, f.mean, f.cov, f.C
    st.weights[:] = f.weights
    return st


def _first_bad(ok, what):
    bad = np.nonzero(~ok)
    assert len(bad[0]) == 0, "%s: %d entries out of tolerance, the first at particle %d" % (what, len(bad[0]), bad[0][0])


def device_state(nav, stride, bulk=True):
    """(planes[10][P][stride], counts, poses) of the state the handle's getters report. bulk: one phd_download_state_soa;
    a frozen handle (the timed mode) keeps its input as the current state and reports the last step's result through the
    getters only, so there it is read particle by particle (MapModel)."""
    if bulk:
        planes, counts, poses, _ = nav.download_state(stride)
        return planes, counts, poses
    P = nav.particle_count
    planes = np.zeros((10, P, stride))
    counts = np.zeros(P, np.int32)
    for i in range(P):
        w, m, c = nav.MapModel(i)
        n = counts[i] = len(w)
        assert n <= stride
        planes[0, i, :n] = w
        planes[1:4, i, :n] = m.T
        for t, (a, b) in enumerate(_UT):
            planes[4 + t, i, :n] = c[:, a, b]
    return planes, counts, nav.poses()


def assert_step_matches(nav, st, best, src, res, stride, what, bulk=True):
    """the handle's state after a step against the oracle's (st, and orc.slam_update's best / src / res); bulk: see
    device_state"""
    gsrc, gres = nav.resample_sources()
    assert gres == res, "%s: resampling decision %s, the oracle's %s" % (what, gres, res)
    if not np.array_equal(gsrc, src):
        i = int(np.nonzero(np.asarray(gsrc) != src)[0][0])
        raise AssertionError("%s: resampling sources differ, first at %d: %d vs %d" % (what, i, gsrc[i], src[i]))
    assert nav.BestParticle == best, "%s: BestParticle %d, the oracle's %d" % (what, nav.BestParticle, best)
    w = nav.VehicleWeights
    assert np.array_equal(np.isnan(w), np.isnan(st.weights)) and np.array_equal(w == 0, st.weights == 0), \
        "%s: zero / NaN particle weights differ" % what
    _first_bad(np.isclose(w, st.weights, rtol=1e-6, atol=1e-300, equal_nan=True), what + ": particle weights")
    planes, counts, poses = device_state(nav, stride, bulk)
    assert np.array_equal(poses, st.poses), "%s: poses differ" % what
    if not np.array_equal(counts, st.n):
        i = int(np.nonzero(counts != st.n)[0][0])
        raise AssertionError("%s: map of particle %d has %d components, the oracle's %d" % (what, i, counts[i], st.n[i]))
    n = min(stride, st.cap)
    assert counts.max() <= n
    mask = np.arange(n)[None, :] < counts[:, None]
    gw, ow = planes[0, :, :n], st.w[:, :n]
    _first_bad(np.isclose(gw, ow, rtol=1e-7, atol=1e-12) | ~mask, what + ": map weights")
    for k in range(3):
        _first_bad(np.isclose(planes[1 + k, :, :n], st.mean[:, :n, k], rtol=1e-7, atol=1e-11) | ~mask, what + ": map means")
    for t, (a, b) in enumerate(_UT):
        _first_bad(np.isclose(planes[4 + t, :, :n], st.cov[:, :n, a, b], rtol=1e-7, atol=1e-13) | ~mask, what + ": map covariances")
    # the best map estimate of BestParticle (what a host plots): OSPA against the oracle's
    b = nav.BestParticle
    cov = np.zeros((counts[b], 3, 3))
    for t, (i, j) in enumerate(_UT):
        cov[:, i, j] = cov[:, j, i] = planes[4 + t, b, :counts[b]]
    glm, _ = orc.best_map_estimate((planes[0, b, :counts[b]], planes[1:4, b, :counts[b]].T, cov))
    olm, _ = orc.best_map_estimate(st.map(best))
    d, card = orc.ospa(glm, olm)
    assert card == 0 and d < 1e-4, "%s: OSPA of the best map estimate %g (cardinality part %g)" % (what, d, card)
