"""The density sums of WeightAlpha (alpha_density_body) at every map-estimate size J at which the lane layout of its pair loop
changes: for J <= 128 a lane holds two landmarks of a block of S slots (S = 64, or the power of two the last block's remainder
rounds up to) and the 2 * 64 / S lane groups of a wave take different components; a block of one slot keeps one landmark per lane;
J = 0 and J > 128 keep the landmark-per-lane loop. The layout changes the ORDER of a sum of non-negative terms and nothing else,
so the tolerances are those of tests/test_gpu_parity.py for the same quantities: alpha against orc.weight_alpha at rtol 1e-6, the
set log-likelihood at 1e-9 — and the order is a fixed function of (J, the counts, the lane): the separate kernels, the one-launch
chain with helper workgroups and the chain without them must give the same bits.

How J is set. J = floor(total weight of the pruned corrected map) (BestMapEstimate). The frame: 4 particles, 12 measurements, 8
visible prior components of weight ~0.05 and J / 0.9 more beyond the range clip (detection probability 0: the misdetection copy keeps
the whole weight and no detection update is made of them); the clutter density is 1, so that the detection updates of the visible
components and of the births weigh little and the total follows the prior weights. The weights beyond the clip are u_c * s with
u_c ~ U(0.85, 1) fixed by the seed and ONE scale s, found with the oracle so that every particle's total lies well inside
(J, J + 1); the J the oracle then finds is asserted, so that a case cannot silently test another size."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import orc
from monorfs_amd.abi import prm3d_defaults
from monorfs_amd.synth import Frame

SIZES = [0, 1, 2, 3, 16, 17, 32, 33, 63, 64, 65, 66, 80, 81, 96, 97, 127, 128, 129]
NVIS = 8
FAR_COV = 100.0
MODES = {   # the way tests/test_gpu_round5.py and tests/test_gpu_parity.py select them
    "kernels": {"PHD_CHAIN_MAX": "0", "PHD_SPLIT": "2", "PHD_DSPLIT_MAX": None},
    "chain, helpers": {"PHD_CHAIN_MAX": None, "PHD_SPLIT": None, "PHD_DSPLIT_MAX": "256"},
    "chain, no helpers": {"PHD_CHAIN_MAX": None, "PHD_SPLIT": None, "PHD_DSPLIT_MAX": "0"},
}


@pytest.fixture(scope="module")
def nav_mod():
    from monorfs_amd import navigator
    return navigator


def _params(f, **over):
    p = prm3d_defaults(max_particles=f.P, max_components=600, max_measurements=max(f.M, 1))
    for k, v in over.items():
        setattr(p, k, v)
    return p


def _oracle(p, f):
    """per particle: (predicted, pruned corrected) mixtures of the oracle"""
    out = []
    for i in range(f.P):
        pred = orc.predict(p, f.poses[i], f.z, f.map(i))
        out.append((pred, orc.prune(p, orc.correct(p, f.poses[i], f.z, pred))))
    return out


def _reference(p, f, mixes):
    alpha, setll, Js = [], [], []
    for i, (pred, pr) in enumerate(mixes):
        a, sll = orc.weight_alpha(p, f.poses[i], f.z, pred, pr)
        alpha.append(a)
        setll.append(sll)
        Js.append(len(orc.best_map_estimate(pr)[0]))
    return np.array(alpha), np.array(setll), Js


@functools.lru_cache(maxsize=None)
def _sized_case(J, far_cov=FAR_COV):
    """(frame, params, oracle alpha, oracle set log-likelihood, the oracle's J per particle) — computed once per size"""
    C = NVIS + max(2, int(np.ceil(J / 0.9)))
    f = Frame(4, C, 12, 7000 + J, weight_profile="steady")
    rng = np.random.default_rng(9000 + J)
    far = np.arange(C) >= NVIS
    rngs = np.linalg.norm(f.mean[:, far], axis=2, keepdims=True)
    f.mean[:, far] *= rng.uniform(2.5, 3.5, (1, int(far.sum()), 1)) / rngs     # range clip: 2 m
    f.cov = np.array(f.cov)
    f.cov[:, far] *= far_cov      # wide enough to overlap: a landmark's density is a sum of many comparable terms
    u = rng.uniform(0.85, 1.0, C)
    p = _params(f, clutter_density=1.0)
    s = (J + 0.5) / u[far].sum()
    for _ in range(12):
        f.w = np.broadcast_to(np.where(far, u * s, 0.05 * u), (4, C)).copy()
        mixes = _oracle(p, f)
        tot = np.array([pr[0].sum() for _, pr in mixes])
        if tot.min() > J + 0.15 and tot.max() < J + 0.85:
            break
        s *= (J + 0.5) / tot.mean()
    return (f, p) + _reference(p, f, mixes)


def _device(nav_mod, monkeypatch, f, p):
    """alpha and the set log-likelihood of the stage run, weights / resampling sources / resampled of one SlamUpdate, per mode"""
    got = {}
    for mode, env in MODES.items():
        for k, v in env.items():
            if v is None:
                monkeypatch.delenv(k, raising=False)
            else:
                monkeypatch.setenv(k, v)
        nav = nav_mod.PHDNavigator(p, particlecount=f.P)
        nav.upload_state(f.planes(), f.counts, f.poses, f.weights)
        nav.run_stages(f.z)
        alpha, setll = nav.WeightAlpha(), nav.SetLogLikelihood()
        nav.SlamUpdate(None, f.z, u_resample=0.3)
        got[mode] = (alpha, setll, nav.VehicleWeights) + nav.resample_sources()
        nav.close()
    for k in ("PHD_CHAIN_MAX", "PHD_SPLIT", "PHD_DSPLIT_MAX"):
        monkeypatch.delenv(k, raising=False)
    return got


def _check(nav_mod, monkeypatch, f, p, alpha, setll):
    assert np.all(np.isfinite(alpha)) and np.all(alpha > 0), "the oracle's alpha underflows: the case compares nothing (%r)" % (alpha,)
    got = _device(nav_mod, monkeypatch, f, p)
    st = orc.State(f.P, 700)
    st.poses[:] = f.poses
    st.w[:, :f.C], st.mean[:, :f.C], st.cov[:, :f.C], st.n[:] = f.w, f.mean, f.cov, f.C
    _, src, res, _ = orc.slam_update(p, st, f.z, u=0.3, threads=4)
    for mode, (ga, gs, gw, gsrc, gres) in got.items():
        print(mode, "alpha max rel", np.max(np.abs(ga - alpha) / alpha), "setll max abs", np.max(np.abs(gs - setll)),
              "weights max rel", np.max(np.abs(gw - st.weights) / st.weights))
    for mode, (ga, gs, gw, gsrc, gres) in got.items():
        assert np.allclose(gs, setll, rtol=1e-9, atol=1e-9), "%s: set log-likelihood %r vs %r" % (mode, gs, setll)
        assert np.allclose(ga, alpha, rtol=1e-6, atol=0), "%s: alpha %r vs %r" % (mode, ga, alpha)
        assert gres == res and np.array_equal(gsrc, src), "%s: resampling differs from the oracle" % mode
        assert np.allclose(gw, st.weights, rtol=1e-6, atol=1e-300), "%s: weights %r vs %r" % (mode, gw, st.weights)
    ref = got["kernels"]
    for mode in ("chain, helpers", "chain, no helpers"):
        for what, a, b in zip(("alpha", "set log-likelihood", "weights", "sources"), got[mode], ref):
            assert np.array_equal(a, b), "%s differs in its bits between '%s' and the separate kernels" % (what, mode)


@pytest.mark.parametrize("J", SIZES)
def test_density_sums_at_every_size_the_layout_changes(nav_mod, monkeypatch, J):
    f, p, alpha, setll, Js = _sized_case(J)
    assert Js == [J] * f.P, "the oracle's map estimates have %r landmarks, the case is built for %d" % (Js, J)
    _check(nav_mod, monkeypatch, f, p, alpha, setll)


def test_corrected_map_of_misdetection_copies_only(nav_mod, monkeypatch):
    """No measurement: no birth, no detection update — the corrected map is the predicted components' misdetection copies, all of them
    accounted for by the first sweep's weight ratios; the second sweep has nothing to add. Two landmark blocks (J = 70)."""
    f0, _, _, _, _ = _sized_case(70, 1.0)   # (narrow components: none close enough to another to be merged)
    f = Frame(4, f0.C, 0, 7070, weight_profile="steady")
    f.mean, f.cov, f.w = f0.mean.copy(), f0.cov.copy(), f0.w.copy()
    p = _params(f, clutter_density=1.0)
    mixes = _oracle(p, f)
    alpha, setll, Js = _reference(p, f, mixes)
    for pred, pr in mixes:
        assert len(pred[0]) == f.C and len(pr[0]) == f.C, "a birth, a detection update or a merge: not the case this test is for"
    assert min(Js) > 64 and max(Js) <= 128, Js
    _check(nav_mod, monkeypatch, f, p, alpha, setll)


def test_corrected_map_without_any_misdetection_copy(nav_mod, monkeypatch):
    """Every prior weight below MinWeight and every measurement a detection of a prior component (no clutter, hence no birth): no
    misdetection copy survives PruneModel — every weight ratio of the first sweep is 0 — and the corrected map is made of detection
    updates alone, all of them left to the second sweep."""
    f = Frame(4, 20, 12, 7171, detect_fraction=1.0, weight_profile="steady")
    p = _params(f)
    f.w = np.full((4, 20), 0.9 * p.min_weight)
    mixes = _oracle(p, f)
    alpha, setll, Js = _reference(p, f, mixes)
    for pred, pr in mixes:
        assert len(pred[0]) == f.C, "a birth: its misdetection copy would survive"
        # (a copy weighs (1 - PD) w <= w < MinWeight: PruneModel's cut comes before its merge)
        assert f.w.max() < p.min_weight and len(pr[0]) > 0 and pr[0].min() >= p.min_weight, "a misdetection copy survived the prune"
    assert min(Js) >= 2, Js
    _check(nav_mod, monkeypatch, f, p, alpha, setll)
