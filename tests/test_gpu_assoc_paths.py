"""The association body (alpha_assoc_body, phd_alpha.h) on every path of BestMapEstimate and SetLogLikelihood that its phases
distinguish: the sizes of the map estimate at which an array moves or a loop changes, the orderings of the selected weights (all
distinct, hundreds exactly equal in the threshold bin of the select, runs of equal weights among the selected), the merge of the
(w - 1) copies, an expected size next to an integer, the shapes of the gating graph that min-label propagation walks, and the
measurement counts at the edges of a block of 64.

Each case of the filter is checked four ways: the set log-likelihood against the oracle at 1e-9, alpha at 1e-6 (the tolerances of
tests/test_gpu_parity.py), the map estimate, and the same bits from the separate kernels, the one-launch chain with helper workgroups
and the chain without them (tests/test_gpu_density_layout.py's `_check`, which also compares one whole SlamUpdate).

The map estimate. The device keeps the landmark list in its own scratch and the ABI has no getter for it, so the list is checked
through what is computed FROM it: the oracle's list (orc.best_map_estimate, in order) is put through orc.set_log_likelihood, which
must reproduce the oracle's own value, and the device's value must agree with that to 1e-9; its length J is asserted; and where a
case is about WHICH components are picked it is built so that the list another rule would give (`_witness` and the rules above
it) moves the set log-likelihood by far more than the tolerance. The order of the list moves only the order of the sum over the
clusters, which the 1e-9 covers and the equal bits of the three modes pin down.

The gating graphs with a prescribed shape (a chain that needs several iterations, laid out with ascending and with descending
landmark indices) go through the quasi set log-likelihood, which takes the landmark list as an argument and runs the same gate,
label propagation and cluster sums; its value and gradient are compared with the references tests/test_gpu_kat.py compares with."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import orc
from monorfs_amd.abi import prm3d_defaults
from monorfs_amd.synth import measure_perfect_identity, measure_to_map_identity
from test_gpu_density_layout import _check, _oracle, _params, _reference, _sized_case, nav_mod  # noqa: F401 (nav_mod: a fixture)
from test_gpu_shape_edges import alpha_frame, seq_sum, tuned

PD = 0.2   # (test_gpu_shape_edges.py: a few hundred undetected landmarks keep alpha far above the smallest double)


def _p(f, **over):
    return _params(f, pd=PD, **over)


def _estimates(p, f, mixes):
    """per particle: the oracle's landmark list, the indices it picked, and the set log-likelihood of that list"""
    out = []
    for i, (_, pr) in enumerate(mixes):
        lm, src = orc.best_map_estimate(pr)
        out.append((lm, src, orc.set_log_likelihood(p, f.poses[i], lm, f.z)))
    return out


def next_best(pr, lm, src):
    """the estimate with its last pick replaced by the heaviest component that was not picked at all"""
    left = [c for c in np.argsort(-pr[0], kind="stable") if c not in set(src.tolist())]
    alt = lm.copy()
    alt[-1] = pr[1][left[0]]
    return alt


def heaviest_as_they_are(pr, lm, src):
    """the J heaviest components, each once: the estimate if the (w - 1) copies were not merged in"""
    return pr[1][np.argsort(-pr[0], kind="stable")[:len(lm)]]


def ties_by_descending_index(pr, lm, src):
    """the J heaviest with equal weights taken from the END of the map"""
    n = len(pr[0])
    return pr[1][np.lexsort((-np.arange(n), -pr[0]))[:len(lm)]]


def _witness(p, f, mixes, i, other):
    """|change of the set log-likelihood| of particle i when its estimate is replaced by the list `other` builds"""
    pr = mixes[i][1]
    lm, src = orc.best_map_estimate(pr)
    alt = other(pr, lm, src)
    assert len(alt) == len(lm)
    return abs(orc.set_log_likelihood(p, f.poses[i], alt, f.z)[0] - orc.set_log_likelihood(p, f.poses[i], lm, f.z)[0])


def _run(nav_mod, monkeypatch, f, p, J=None, witness=None, built=None):
    mixes, (alpha, setll, Js) = built if built is not None else _built(p, f)
    if J is not None:
        assert Js == [J] * f.P, "the oracle's map estimates have %r landmarks, the case is built for %r" % (Js, J)
    for i, (lm, src, (v, ncl, mx)) in enumerate(_estimates(p, f, mixes)):
        assert len(lm) == Js[i] and abs(v - setll[i]) <= 1e-9 * max(1.0, abs(v)), "the oracle's list does not give the oracle's value"
    if witness:
        for i in range(f.P):
            d = _witness(p, f, mixes, i, witness)
            assert d > 1e-3, "particle %d: another pick would not show in the set log-likelihood (%r)" % (i, d)
    _check(nav_mod, monkeypatch, f, p, alpha, setll)
    return Js


def _built(p, f):
    mixes = _oracle(p, f)
    return mixes, _reference(p, f, mixes)


# ---- the sizes of the map estimate ------------------------------------------------------------------------------------------
# 0, 1, 4: the literal enumeration below five landmarks; 5 - 9: every tail of a wave's stride of four over the landmarks;
# 63 - 65, 128, 129: a block of 64, and the 128 up to which two threads share a landmark's logarithms; 256 / 257: LDS arrays
# against the HBM slab
SIZES = [0, 1, 4, 5, 6, 7, 8, 9, 63, 64, 65, 128, 129, 256, 257]


@pytest.mark.parametrize("J", SIZES)
def test_map_estimate_sizes(nav_mod, monkeypatch, J):   # noqa: F811
    """tests/test_gpu_density_layout.py's frame: J / 0.9 components of distinct weights beyond the range clip, 8 in view"""
    f, p, alpha, setll, Js = _sized_case(J)
    mixes = _oracle(p, f)
    _run(nav_mod, monkeypatch, f, p, J, built=(mixes, (alpha, setll, Js)))


def test_more_landmarks_than_components(nav_mod, monkeypatch):   # noqa: F811
    """J = 13 from 7 components (three in view at 4.3 after the correction, each picked five times): the whole list is sorted
    (the bitonic path) and merged with the (w - 1) copies"""
    p = prm3d_defaults(max_particles=2, max_components=600, max_measurements=1)
    p.pd = PD
    f = tuned(p, alpha_frame(3, 5.375, 0, np.full(4, 0.01), 4601), 4, 13.5)
    mixes, ref = _built(p, f)
    assert all(len(pr[0]) < 13 for _, pr in mixes)
    _run(nav_mod, monkeypatch, f, p, 13, built=(mixes, ref))


# ---- the rankings ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _equal_bin_case(need, n_eq=300, n_det=6, n_out=12):
    """n_eq components in view of ONE prior weight: their misdetection copies weigh exactly the same ((1 - PD) w, PD constant
    inside the film), so they share a bin of the select's histogram and only the map index orders them. The n_det detection
    updates and n_out components beyond the film's edge (which keep their prior weight, tuned here) are heavier: `above` of the
    bins above, and the expected size is put at above + need + 0.5, so that `need` of the n_eq equal ones are picked. The first
    n_det components are the measured ones: whether a measured one is among the picks decides a cluster of the set
    log-likelihood, which is the witness of the tie-break."""
    if need == n_eq:   # all of them: nothing heavier, nothing measured, the rest light
        e, n_det, wo = 1.0005, 0, np.full(n_out, 0.03)
    else:              # (300 e = need + 0.6: what is heavier then sums to just under its count, and nothing exceeds 1 + e)
        e, wo = (need + 0.6) / n_eq, np.full(n_out, 0.99)
    f0 = alpha_frame(n_eq, e / (1 - PD), n_det, wo, 4900 + need, P=2)
    p = _p(f0, max_measurements=max(n_det, 1))
    f = f0
    for _ in range(6):
        pw = [pr[0] for _, pr in _oracle(p, f)]
        eq = [np.sum(w == np.median(w)) for w in pw]
        above = [int(np.sum(w > np.median(w))) for w in pw]
        assert len(set(above)) == 1 and min(eq) > 256, (above, eq)
        g = tuned(p, f, n_out, above[0] + need + 0.5)
        assert g is not None
        if g is f:
            break
        f = g
        tot = [seq_sum(pr[0]) for _, pr in _oracle(p, f)]
        if all(abs(t - (above[0] + need + 0.5)) < 0.3 for t in tot):
            break
    mixes, ref = _built(p, f)
    for (_, pr), j in zip(mixes, ref[2]):
        w = pr[0]
        med = np.median(w)
        assert np.sum(w == med) > 256 and j - int(np.sum(w > med)) == need, (np.sum(w == med), j, int(np.sum(w > med)), need)
        ws = np.sort(w)[::-1]
        assert not (ws[0] - 1 > ws[j - 1]), "the merge path: not this case"
    return f, p, mixes, ref


@pytest.mark.parametrize("need", [1, 150, 300])
def test_threshold_bin_of_equal_weights(nav_mod, monkeypatch, need):   # noqa: F811
    """more than 256 exactly equal weights in the threshold bin, of which the first 1, the first half and all are taken"""
    f, p, mixes, ref = _equal_bin_case(need)
    _run(nav_mod, monkeypatch, f, p, witness=ties_by_descending_index if need < 300 else None, built=(mixes, ref))


def test_runs_of_equal_weights_among_the_selected(nav_mod, monkeypatch):   # noqa: F811
    """the selected weights come in runs of equal values (22 and 23 long, so that the runs straddle every quarter and every
    multiple of 64 of the list); 90 components beyond the film's edge and 6 measured ones in view"""
    wo = np.repeat([1.04, 1.0, 0.93, 0.81], [22, 23, 22, 23])
    f = alpha_frame(6, 1.1, 6, wo, 4950, P=2)
    p = _p(f)
    mixes, ref = _built(p, f)
    assert min(ref[2]) > 64 and all(j <= len(pr[0]) for (_, pr), j in zip(mixes, ref[2]))
    _run(nav_mod, monkeypatch, f, p, built=(mixes, ref))


def test_merge_of_the_reduced_copies(nav_mod, monkeypatch):   # noqa: F811
    """two components in view at 2.56 after the correction, thirty of 0.4 beyond the film: the heaviest minus one exceeds the J-th
    weight, the estimate takes each of the two three times (2.56, 1.56, 0.56) — six undetected landmarks in view, against two if
    the J heaviest were taken as they are"""
    f = alpha_frame(2, 2.56 / (1 - PD), 0, np.full(30, 0.4), 4960, P=2)
    p = _p(f, max_measurements=1)
    f = tuned(p, f, 30, 17.5)
    mixes, ref = _built(p, f)
    for (_, pr), j in zip(mixes, ref[2]):
        ws = np.sort(pr[0])[::-1]
        assert j <= len(ws) and ws[0] - 1 > ws[j - 1], "not the merge path"
        _, src = orc.best_map_estimate(pr)
        assert len(set(src.tolist())) < len(src), "no component is picked twice"
    _run(nav_mod, monkeypatch, f, p, 17, witness=heaviest_as_they_are, built=(mixes, ref))


@pytest.mark.parametrize("side", ["below", "above"])
def test_expected_size_next_to_an_integer(nav_mod, monkeypatch, side):   # noqa: F811
    """the sum of the weights in map order within 1e-9 of 40, from below (J = 39) and from above (J = 40): the block sum is then
    re-added by one thread in map order"""
    J, n_out = 40, 60
    target = J - 4e-10 if side == "below" else J + 4e-10
    rng = np.random.default_rng(4970)
    f0 = alpha_frame(44, 1.1, 0, rng.uniform(0.01, 0.04, n_out), 4970, P=1)
    p = _p(f0, max_measurements=1)
    f = tuned(p, f0, n_out, target)
    for _ in range(8):
        s = seq_sum(_oracle(p, f)[0][1][0])
        if abs(s - target) < 1e-10:
            break
        w = np.array(f.w[0])
        w[-1] += target - s
        f.w = w[None]
    s = seq_sum(_oracle(p, f)[0][1][0])
    assert abs(s - J) <= 1e-9 * J and (s < J) == (side == "below"), s - J
    _run(nav_mod, monkeypatch, f, p, J - 1 if side == "below" else J)


# ---- the gating graph -------------------------------------------------------------------------------------------------------
def test_no_gated_pair(nav_mod, monkeypatch):   # noqa: F811
    """no measurement within the gate of any landmark of the estimate: every landmark and every measurement is a cluster of its
    own and the propagation ends in its first iteration"""
    f = alpha_frame(12, 1.1, 0, np.full(20, 0.5), 4980, P=2)
    p = _p(f, max_measurements=8, clutter_density=1.0)   # (births and detection updates weigh little: none is picked)
    rng = np.random.default_rng(4980)
    f.M = 8
    f.z = np.stack([rng.uniform(-300, 300, 8), rng.uniform(215, 235, 8), np.full(8, 1.95)], axis=1)   # (the grid ends at y = 200, ranges at 1.6)
    mixes, ref = _built(p, f)
    for i, (lm, src, (v, ncl, mx)) in enumerate(_estimates(p, f, mixes)):
        assert mx <= 1 and ref[2][i] >= 5, (mx, ref[2][i])
    _run(nav_mod, monkeypatch, f, p, built=(mixes, ref))


def test_every_measurement_gated_with_a_landmark(nav_mod, monkeypatch):   # noqa: F811
    """24 measured components, all of them in the estimate: every measurement lies in the gate of a landmark"""
    f = alpha_frame(24, 1.1, 24, np.full(10, 0.3), 4990, P=2)
    p = _p(f)
    mixes, ref = _built(p, f)
    for i, (lm, src, (v, ncl, mx)) in enumerate(_estimates(p, f, mixes)):
        zh = np.array([orc.measure_perfect(p, f.poses[i], m) for m in lm])
        d = (zh[None] - f.z[:, None]) / np.sqrt([2.0, 2.0, 1e-3])
        assert np.all(np.min(np.sum(d * d, axis=2), axis=1) < 25.0), "a measurement without a landmark in its gate"
    _run(nav_mod, monkeypatch, f, p, witness=next_best, built=(mixes, ref))


@pytest.mark.parametrize("M", [1, 63, 64, 65])
def test_measurement_block_edges(nav_mod, monkeypatch, M):   # noqa: F811
    """one measurement, a block of 64 less one, exactly one, and one more (two blocks per landmark in the gate loop)"""
    f = alpha_frame(max(M, 8) + 4, 1.1, M, np.full(10, 0.3), 5000 + M, P=2)
    p = _p(f)
    _run(nav_mod, monkeypatch, f, p)


# ---- prescribed graphs, through the quasi set log-likelihood -------------------------------------------------------------------
def _chain(n, descending):
    """n landmarks 30 pixels apart at one range and n - 1 measurements half-way between neighbours: under the quasi gate (12
    sigma: 17 pixels) a measurement is gated with its two neighbours only, and the smallest label needs about n iterations to reach
    the far end — against the index order or along it"""
    zl = np.stack([-150.0 + 30.0 * np.arange(n), np.full(n, 20.0), np.full(n, 1.0)], axis=1)
    zm = 0.5 * (zl[1:] + zl[:-1])
    lm = measure_to_map_identity(zl)
    if descending:
        lm = lm[::-1].copy()
    return lm, zm


@pytest.fixture(scope="module")
def qnav():
    from monorfs_amd import navigator
    p = prm3d_defaults(max_particles=8, max_components=600, max_measurements=16)
    n = navigator.PHDNavigator(p, particlecount=1)
    yield n
    n.close()


@pytest.mark.parametrize("descending", [False, True])
def test_chain_of_landmarks_sharing_one_measurement_each(qnav, descending):
    lm, zm = _chain(8, descending)
    rng = np.random.default_rng(5100)
    poses = np.zeros((4, 7))
    poses[:, 3] = 1
    poses[1:, :3] = rng.normal(0, 1e-3, (3, 3))
    p = qnav.params
    zh = measure_perfect_identity(lm)
    d = (zh[None] - zm[:, None]) / np.sqrt([2.0, 2.0, 1e-3])
    assert np.all(np.sum(np.sum(d * d, axis=2) < 144.0, axis=1) == 2), "a measurement is not gated with exactly its two neighbours"
    got = qnav.QuasiSetLogLikelihood(zm, lm, poses)
    want = np.array([orc.quasi_set_log_likelihood(p, q, lm, zm) for q in poses])
    assert np.all(np.isfinite(want)) and np.allclose(got, want, rtol=1e-9, atol=1e-9), (got, want)
    # the two layouts are the same set of landmarks
    other, _ = _chain(8, not descending)
    assert np.allclose(qnav.QuasiSetLogLikelihood(zm, other, poses), got, rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("mode", [0, 1])
def test_quasi_value_and_gradient_on_a_frame_of_the_filter(qnav, mode):
    """the landmarks of the `every measurement gated` frame's estimate and its measurements: value and gradient against the oracle
    (the tolerances of tests/test_gpu_kat.py)"""
    f = alpha_frame(24, 1.1, 12, np.full(10, 0.3), 4990, P=2)
    p = _p(f)
    lm, _ = orc.best_map_estimate(_oracle(p, f)[0][1])
    assert len(lm) >= 12
    rng = np.random.default_rng(5200)
    poses = np.concatenate([f.poses, f.poses + np.concatenate([rng.normal(0, 2e-3, (2, 3)), np.zeros((2, 4))], axis=1)])
    q = qnav.params
    L, G = qnav.QuasiSetLogLikelihoodGradient(f.z, lm, poses, average_mode=mode)
    for i, pose in enumerate(poses):
        v, g = orc.quasi_set_log_likelihood_grad(q, pose, lm, f.z, mode)
        assert np.isclose(L[i], v, rtol=1e-11, atol=1e-11) and np.allclose(G[i], g, rtol=1e-9, atol=1e-9), (i, L[i], v, G[i], g)
    assert np.array_equal(qnav.QuasiSetLogLikelihood(f.z, lm, poses), L)
