"""The density sums of WeightAlpha (alpha_density_body) for map estimates of 80 < J <= 96 landmarks: one block of 96 slots, lane
jl = lane & 31 holds the landmarks jl, 32 + jl and 64 + jl and reads a staged record once for the three; and the second sweep
takes its components — the entries of the pruned corrected map that are no misdetection copy of a predicted component, "uncovered"
below — from ONE list over the whole map, staged in tiles of 256 list entries, instead of one compaction per window of 256 map
entries. As in tests/test_gpu_density_layout.py, whose frames, modes and checks these cases use, this changes the order of sums
of non-negative terms and nothing else: alpha and the weights against the oracle at rtol 1e-6, the set log-likelihood at 1e-9
(tests/test_gpu_parity.py), and the same bits from the separate kernels, the chain with helper workgroups and the chain without.

Every case asserts from the oracle what it means to test: the J of every particle, and the uncovered count of its pruned map —
the entries whose moments are not a predicted component's, by the rule k_prune_merge marks them with (means within 1e-9
relative, covariances within 1e-9 of the largest diagonal entry)."""
import functools

import numpy as np
import pytest

import orc

pytestmark = pytest.mark.gpu

from monorfs_amd.synth import Frame
from test_gpu_density_layout import _check, _oracle, _params, _reference, _sized_case, nav_mod  # noqa: F401  (nav_mod: the fixture)

LO, HI = 80, 96   # the triple layout: LO < J <= HI
FAR_COV_LONG, NLIGHT_LONG = 4.0, 1950


def _uncovered(pred, pruned):
    pm, pc = pred[1], pred[2].reshape(len(pred[1]), -1)
    n = 0
    for m, c in zip(pruned[1], pruned[2]):
        c = c.reshape(-1)
        same = np.all(np.abs(pm - m) <= 1e-9 * np.abs(m), axis=1) & np.all(np.abs(pc - c) <= 1e-9 * max(abs(c[0]), abs(c[4]), abs(c[8])), axis=1)
        n += not same.any()
    return n


def _counts(mixes):
    """per particle: predicted components, entries of the pruned corrected map, uncovered entries"""
    return [len(pred[0]) for pred, _ in mixes], [len(pr[0]) for _, pr in mixes], [_uncovered(pred, pr) for pred, pr in mixes]


def _with_measurements(f0, M, seed):
    """the map of frame f0 under M measurements of another draw"""
    f = Frame(4, f0.C, M, seed, weight_profile="steady")
    f.mean, f.cov, f.w = f0.mean.copy(), np.array(f0.cov), f0.w.copy()
    return f


@functools.lru_cache(maxsize=None)
def _built_case(J, nvis, M, vis_cov, pad, clutter, seed):
    """The frame of test_gpu_density_layout._sized_case with three more knobs: `nvis` visible components whose covariances are
    scaled by `vis_cov` (wide ones pair with every measurement), `pad` further components beyond the range clip whose weight,
    half of MinWeight, does not survive the prune (they lengthen the predicted mixture and nothing else), the clutter density."""
    nfar = max(2, int(np.ceil(J / 0.9)))
    C = nvis + nfar + pad
    f = Frame(4, C, M, seed, weight_profile="steady")
    rng = np.random.default_rng(seed + 1)
    idx = np.arange(C)
    far, padded = idx >= nvis, idx >= nvis + nfar
    rngs = np.linalg.norm(f.mean[:, far], axis=2, keepdims=True)
    f.mean[:, far] *= rng.uniform(2.5, 3.5, (1, int(far.sum()), 1)) / rngs     # range clip: 2 m
    f.cov = np.array(f.cov)
    f.cov[:, far] *= 100.0
    f.cov[:, ~far] *= vis_cov
    u = rng.uniform(0.85, 1.0, C)
    p = _params(f, clutter_density=clutter)
    s = (J + 0.5) / u[far & ~padded].sum()
    for _ in range(12):
        f.w = np.broadcast_to(np.where(padded, 0.5 * p.min_weight, np.where(far, u * s, 0.05 * u)), (4, C)).copy()
        mixes = _oracle(p, f)
        tot = np.array([pr[0].sum() for _, pr in mixes])
        if tot.min() > J + 0.15 and tot.max() < J + 0.85:
            break
        s *= (J + 0.5) / tot.mean()
    return f, p, mixes


def _inside(Js):
    assert LO < min(Js) and max(Js) <= HI, "the oracle's map estimates have %r landmarks: not the triple layout's sizes" % (Js,)


@pytest.mark.parametrize("J", [82, 88, 95])
def test_density_sums_inside_the_triple_range(nav_mod, monkeypatch, J):
    f, p, alpha, setll, Js = _sized_case(J)
    assert Js == [J] * f.P, "the oracle's map estimates have %r landmarks, the case is built for %d" % (Js, J)
    _check(nav_mod, monkeypatch, f, p, alpha, setll)


def test_no_uncovered_entry(nav_mod, monkeypatch):
    """No measurement: the corrected map is the predicted components' misdetection copies — the list is empty."""
    f = _with_measurements(_sized_case(88, 1.0)[0], 0, 7088)   # (narrow components: none close enough to another to be merged)
    p = _params(f, clutter_density=1.0)
    mixes = _oracle(p, f)
    alpha, setll, Js = _reference(p, f, mixes)
    _inside(Js)
    assert _counts(mixes)[2] == [0] * f.P, _counts(mixes)
    _check(nav_mod, monkeypatch, f, p, alpha, setll)


def test_one_uncovered_entry(nav_mod, monkeypatch):
    """One measurement, the detection of one visible component: its update is the corrected map's only other entry."""
    f = _with_measurements(_sized_case(88, 1.0)[0], 1, 7088)
    p = _params(f)
    mixes = _oracle(p, f)
    alpha, setll, Js = _reference(p, f, mixes)
    _inside(Js)
    assert _counts(mixes)[2] == [1] * f.P, _counts(mixes)
    _check(nav_mod, monkeypatch, f, p, alpha, setll)


def test_no_misdetection_copy_and_one_tile(nav_mod, monkeypatch):
    """Every prior weight 9 MinWeight and visible (a copy weighs 0.1 of it and is cut), 96 measurements, each the detection of a
    component: the corrected map is detection updates alone, every entry is on the list, and the list is one tile."""
    f = Frame(4, 100, 96, 7177, detect_fraction=1.0, weight_profile="steady")
    p = _params(f, min_weight=0.03)   # (MinWeight 0.03: the prior then weighs enough against the updates for alpha not to underflow)
    f.cov = np.array(f.cov) * 0.25
    f.w = np.full((4, 100), 9.0 * p.min_weight)
    mixes = _oracle(p, f)
    alpha, setll, Js = _reference(p, f, mixes)
    _inside(Js)
    _, no, unc = _counts(mixes)
    assert unc == no and 0 < min(no) and max(no) <= 256, (no, unc)
    _check(nav_mod, monkeypatch, f, p, alpha, setll)


def test_uncovered_entries_span_two_tiles(nav_mod, monkeypatch):
    """32 visible components, wide enough to pair with most of 24 measurements above MinWeight: more than 256 detection updates
    between the copies — the list's second tile."""
    f, p, mixes = _built_case(88, 32, 24, 100.0, 0, 3e-7, 7300)
    alpha, setll, Js = _reference(p, f, mixes)
    assert Js == [88] * f.P, Js
    _, no, unc = _counts(mixes)
    assert min(unc) > 256 and max(no) <= 600, (no, unc)
    _check(nav_mod, monkeypatch, f, p, alpha, setll)


def test_births_are_the_last_short_tile(nav_mod, monkeypatch):
    """256 prior components (150 of them too light to survive the prune) and births: the predicted mixture's second tile is the
    births alone."""
    f, p, mixes = _built_case(88, 8, 12, 1.0, 150, 1.0, 7400)
    alpha, setll, Js = _reference(p, f, mixes)
    assert Js == [88] * f.P, Js
    npred, _, unc = _counts(mixes)
    assert f.C == 256 and 256 < min(npred) and max(npred) < 512, npred
    assert min(unc) > 0, unc
    _check(nav_mod, monkeypatch, f, p, alpha, setll)


ULIST = 2048   # entries the list of uncovered components holds (DensLds::ULIST); a longer corrected map keeps the windows of 256


@functools.lru_cache(maxsize=None)
def _long_map_case(J, nvis, M, vis_cov, far_cov, nlight, clutter, seed):
    """_built_case's frame for two particles with `nlight` more components beyond the range clip: light (2 to 2.4 MinWeight, all
    distinct: the prune keeps them, the map estimate does not take them), narrow and spread over 4 - 40 m (none close enough to
    another to be merged). They lengthen the pruned corrected map and nothing else. MaxQuantity and the component capacity are
    raised to `cap`, the next multiple of 64 above the predicted mixture. Returns the corrected mixtures as well."""
    nfar = max(2, int(np.ceil(J / 0.9)))
    C = nvis + nfar + nlight
    f = Frame(2, C, M, seed, weight_profile="steady")
    rng = np.random.default_rng(seed + 1)
    idx = np.arange(C)
    far, light = idx >= nvis, idx >= nvis + nfar
    heavy = far & ~light
    rngs = np.linalg.norm(f.mean, axis=2, keepdims=True)
    f.mean[:, heavy] *= rng.uniform(2.5, 3.5, (1, int(heavy.sum()), 1)) / rngs[:, heavy]     # range clip: 2 m
    f.mean[:, light] *= rng.uniform(4.0, 40.0, (1, nlight, 1)) / rngs[:, light]
    f.cov = np.array(f.cov)
    f.cov[:, heavy] *= far_cov
    f.cov[:, light] *= 0.01
    f.cov[:, ~far] *= vis_cov
    u = rng.uniform(0.85, 1.0, C)
    cap = (C + M + 63) // 64 * 64
    p = _params(f, clutter_density=clutter, max_components=cap, max_quantity=cap)
    wl = 2.0 * p.min_weight * u / 0.85
    s = (J + 0.5 - wl[light].sum()) / u[heavy].sum()
    for _ in range(12):
        f.w = np.broadcast_to(np.where(light, wl, np.where(far, u * s, 0.05 * u)), (2, C)).copy()
        mixes, corrected = [], []
        for i in range(f.P):
            pred = orc.predict(p, f.poses[i], f.z, f.map(i))
            corrected.append(orc.correct(p, f.poses[i], f.z, pred))
            mixes.append((pred, orc.prune(p, corrected[-1])))
        tot = np.array([pr[0].sum() for _, pr in mixes])
        if tot.min() > J + 0.15 and tot.max() < J + 0.85:
            break
        s += (J + 0.5 - tot.mean()) / u[heavy].sum()
    return f, p, mixes, corrected


def _absorbed_rows(p, corrected, pruned):
    """the rows of the prune's cut (the corrected entries of at least MinWeight, heaviest first) that another row absorbed: the
    rows whose mean is no entry's of the pruned map; and the number of rows"""
    w, m = corrected[0], corrected[1]
    keep = w >= p.min_weight
    m = m[keep][np.argsort(-w[keep], kind="stable")][:p.max_quantity]
    gone = [k for k, x in enumerate(m) if np.abs(pruned[1] - x).max(axis=1).min() > 1e-9 * max(1.0, np.abs(x).max())]
    return gone, len(m)


def test_corrected_map_longer_than_the_list(nav_mod, monkeypatch):
    """A pruned corrected map of slightly more than ULIST entries (2 particles, J = 88, some 1950 light components beyond the range
    clip): the list cannot hold their indices, and the triple layout's second sweep falls back to one compaction per window of 256
    map entries. 32 wide visible components under 24 measurements, as in test_uncovered_entries_span_two_tiles: hundreds of
    detection updates that weigh in the corrected density at the landmarks — without the uncovered entries behind the first
    window the oracle's alpha moves by more than a thousand times the tolerance, which is asserted.

    What the case stayed clear of when it was written: a cut of more than 2048 rows in k_prune_merge lost row k + 2048 with every
    absorbed row k (its absorbed flags were one 32-bit word per lane). That limit is gone — the flags are 64 bits per lane, every
    row phd_create admits, held by tests/test_gpu_prune_paths.py. No row below (rows - 2048) is absorbed here, still asserted
    from the oracle's corrected and pruned maps: the density sums are what is tested."""
    f, p, mixes, corrected = _long_map_case(88, 32, 24, 100.0, FAR_COV_LONG, NLIGHT_LONG, 3e-7, 7600)
    alpha, setll, Js = _reference(p, f, mixes)
    assert Js == [88] * f.P, Js
    _, no, unc = _counts(mixes)
    assert min(no) > ULIST and max(no) <= p.max_quantity, no
    for i, (pred, pr) in enumerate(mixes):
        gone, rows = _absorbed_rows(p, corrected[i], pr)
        assert rows > ULIST and all(k >= rows - 2048 for k in gone), (rows, gone[:8])
        # the second sweep matters beyond its first window: alpha without the uncovered entries from map position 256 on
        pm, pc = pred[1], pred[2].reshape(len(pred[1]), -1)
        covered = np.array([bool((np.all(np.abs(pm - m) <= 1e-9 * np.abs(m), axis=1) &
                                  np.all(np.abs(pc - c.reshape(-1)) <= 1e-9 * max(abs(c[0, 0]), abs(c[1, 1]), abs(c[2, 2])), axis=1)).any())
                            for m, c in zip(pr[1], pr[2])])
        sel = covered | (np.arange(len(covered)) < 256)
        assert (~sel).sum() > 0
        a_cut, _ = orc.weight_alpha(p, f.poses[i], f.z, pred, (pr[0][sel], pr[1][sel], pr[2][sel]))
        assert abs(a_cut - alpha[i]) > 1e-3 * alpha[i], (a_cut, alpha[i])
    state = orc.State
    monkeypatch.setattr(orc, "State", lambda P, cap: state(P, max(cap, p.max_components)))   # (_check's oracle state: room for this map)
    _check(nav_mod, monkeypatch, f, p, alpha, setll)


def test_helper_workgroups_stage_ahead(nav_mod, monkeypatch):
    """32 particles (the four of the J = 88 frame, eight times): with helpers on, the chain's helper workgroups stage the first
    tile's prior records before the step has produced anything and then run these sums."""
    f0, p0, _, _, Js = _sized_case(88)
    assert Js == [88] * f0.P, Js
    f = Frame(32, f0.C, f0.M, 7088, weight_profile="steady")
    f.poses, f.z = np.tile(f0.poses, (8, 1)), f0.z.copy()
    f.mean, f.cov, f.w = np.tile(f0.mean, (8, 1, 1)), np.tile(np.array(f0.cov), (8, 1, 1, 1)), np.tile(f0.w, (8, 1))
    p = _params(f, clutter_density=1.0)
    mixes = _oracle(p, f)
    alpha, setll, Js = _reference(p, f, mixes)
    assert Js == [88] * f.P, Js
    _check(nav_mod, monkeypatch, f, p, alpha, setll)
