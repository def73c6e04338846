"""The cut floor of the emit body (phd_correct.h): a step computes only the detection updates that can survive the MaxQuantity
cut of PruneModel, a stage run (phd_stage_run) still emits the whole corrected list down to MinWeight. The two paths check each
other without a switch: after one SlamUpdate the map in slot i must be the stage run's pruned map of resample_sources()[i], bit
for bit, for every particle — on the full-size frames of BASELINE.json, on small frames whose emitted count sits below, at, one
above and far above MaxQuantity (with equal weights straddling the cut), through the one-launch chain and through the separate
kernels, and over an un-frozen sequence against the oracle."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import orc
from monorfs_amd.abi import prm3d_defaults
from monorfs_amd.synth import CONFIGS, Frame
from oracle_parity import assert_step_matches, oracle_state

THREADS = min(16, os.cpu_count() or 1)
_UT = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]


def make_nav(f, maxq):
    from monorfs_amd import navigator
    p = prm3d_defaults(max_particles=f.P, max_components=max(maxq, f.C), max_measurements=f.M)
    p.max_quantity = maxq
    nav = navigator.PHDNavigator(p, particlecount=f.P)
    nav.upload_state(f.planes(), f.counts, f.poses, f.weights)
    return nav, p


def oracle_corrected(p, f, i):
    """the oracle's corrected list of particle i: (size of the predicted mixture, the entries that reach MinWeight in the list's own
    order — the copies first —, the whole list)"""
    pred = orc.predict(p, f.poses[i], f.z, f.map(i))
    cor = orc.correct(p, f.poses[i], f.z, pred)
    keep = ~(cor[0] < p.min_weight)
    return len(pred[0]), keep, cor


def emitted_counts(p, f, particles):
    return np.array([int(oracle_corrected(p, f, i)[1].sum()) for i in particles])


def step_equals_stage_run(f, maxq, u, what, stage_oracle=False):
    """One SlamUpdate of a fresh handle against the stage run of another on the same upload: maps bit for bit (every particle),
    particle weights, resampling and BestParticle against orc.slam_update at the whole-step tolerances of tests/oracle_parity.py
    (the device normalises the weights with its own order of summation: their bits are not reachable from Python).
    stage_oracle: the stage run's pruned maps against orc.prune(orc.correct(orc.predict())) too, every particle, at the stage-parity
    tolerances of tests/test_gpu_parity.py. Returns the stage handle's parameters."""
    from test_gpu_parity import assert_mix_close
    stages, p = make_nav(f, maxq)
    stages.run_stages(f.z, with_alpha=True)
    alpha = stages.WeightAlpha()
    pruned = [stages.PruneModel(i) for i in range(f.P)]
    stages.close()
    if stage_oracle:
        for i in range(f.P):
            _, _, cor = oracle_corrected(p, f, i)
            assert_mix_close(pruned[i], orc.prune(p, cor), 1e-7, "%s: stage run, prune[%d]" % (what, i))
    step, _ = make_nav(f, maxq)
    step.SlamUpdate(None, f.z, u_resample=u)
    src, res = step.resample_sources()
    stride = max(maxq, f.C)
    planes, counts, _, _ = step.download_state(stride)
    for i in range(f.P):
        w, m, c = pruned[int(src[i])]
        n = len(w)
        assert counts[i] == n, "%s: slot %d holds %d components, the stage run's map of particle %d has %d" % (what, i, counts[i], src[i], n)
        same = np.array_equal(planes[0, i, :n], w) and np.array_equal(planes[1:4, i, :n], m.T)
        for t, (a, b) in enumerate(_UT):
            same = same and np.array_equal(planes[4 + t, i, :n], c[:, a, b])
        assert same, "%s: the map in slot %d is not the stage run's pruned map of particle %d, bit for bit" % (what, i, src[i])
    # particle weights, resampling, BestParticle (and every map once more) against the oracle's whole step
    st = oracle_state(f, max(stride, 700))
    best, osrc, ores, oalpha = orc.slam_update(p, st, f.z, u=u, threads=THREADS)
    assert_step_matches(step, st, best, osrc, ores, stride, what)
    assert np.array_equal(alpha == 0, oalpha == 0) and np.allclose(alpha, oalpha, rtol=1e-6, atol=0), "%s: the stage run's WeightAlpha" % what
    step.close()
    return p


# ---- 1. the full-size frames: B and S on both weight profiles, A
@pytest.mark.parametrize("cfg,profile", [("B", "survey"), ("B", "steady"), ("S", "survey"), ("S", "steady"), ("A", "survey"), ("A", "steady")])
def test_step_maps_equal_the_stage_runs_pruned_maps(cfg, profile):
    P, C, M, seed = CONFIGS[cfg]
    f = Frame(P, C, M, seed, weight_profile=profile)
    maxq = max(600, C)
    p = step_equals_stage_run(f, maxq, 0.41, "%s %s" % (cfg, profile))
    # (CPU side: the cut does bite on B and S — the oracle emits more than MaxQuantity entries — and does not on A)
    ne = emitted_counts(p, f, (0, P - 1))
    print("%s %s: the oracle emits %s entries for particles 0 and %d, MaxQuantity %d" % (cfg, profile, ne, P - 1, maxq))
    assert np.all(ne > maxq) if cfg in ("B", "S") else np.all(ne <= maxq)


# ---- 2. the cut boundary and ties, on small frames, through both launch paths
def small_frame(duplicates):
    f = Frame(12, 64, 20, 4242, weight_profile="survey")
    if duplicates:   # the second half of the prior repeats the first: every copy and every detection update comes twice, with equal weights
        h = f.C // 2
        f.mean = np.array(f.mean); f.cov = np.array(f.cov); f.w = np.array(f.w)
        f.mean[:, h:] = f.mean[:, :h]; f.cov[:, h:] = f.cov[:, :h]; f.w[:, h:] = f.w[:, :h]
    return f


def tie_cut(p, f, want_copy):
    """a MaxQuantity at which two EQUAL weights of particle 0 straddle the cut — two misdetection copies (want_copy) or two
    detection updates — or None"""
    npred, keep, cor = oracle_corrected(p, f, 0)
    w = cor[0][keep]
    iscopy = (np.flatnonzero(keep) < npred)
    order = np.lexsort((np.arange(len(w)), -w))   # weight descending, then the list's own order: the reference's sort made stable
    ws, cs = w[order], iscopy[order]
    for K in range(len(w) // 3, len(w) - 1):
        if ws[K - 1] == ws[K] and cs[K - 1] == want_copy and cs[K] == want_copy:
            return K
    return None


BOUNDARY = ["below", "exactly", "one-above", "twice", "tie-copies", "tie-detections"]


@pytest.mark.parametrize("path", ["chain", "separate"])
@pytest.mark.parametrize("case", BOUNDARY)
def test_cut_boundary_and_ties(monkeypatch, case, path):
    """emitted count below K, exactly K, K + 1 and about 2 K; equal weights — copies and detections alike — straddling the cut.
    `path`: the one-launch chain (the default at 12 particles) or the separate kernels (PHD_CHAIN_MAX=0), as in
    test_gpu_round2.test_one_launch_chain_equals_the_separate_kernels."""
    if path == "separate":
        monkeypatch.setenv("PHD_CHAIN_MAX", "0")
    f = small_frame(case.startswith("tie"))
    p0 = prm3d_defaults(max_particles=f.P, max_components=600, max_measurements=f.M)
    ne = emitted_counts(p0, f, range(f.P))   # (MaxQuantity plays no part in the corrected list)
    if case == "below":
        K = int(ne.max()) + 3
        assert np.all(ne < K)
    elif case == "exactly":
        K = int(ne[0])
        assert ne[0] == K
    elif case == "one-above":
        K = int(ne[0]) - 1
        assert ne[0] == K + 1
    elif case == "twice":
        K = int(ne.min()) // 2
        assert np.all(ne >= 2 * K) and K >= 20
    else:
        K = tie_cut(p0, f, case == "tie-copies")
        assert K is not None, "no pair of equal weights of that kind in the frame"
        assert np.all(ne > K), "the oracle does not exceed K emitted entries on every particle"
    print("%s / %s: the oracle emits %d - %d entries, MaxQuantity %d" % (case, path, ne.min(), ne.max(), K))
    step_equals_stage_run(f, K, 0.37, "%s (%s)" % (case, path), stage_oracle=True)


# ---- 3. an un-frozen sequence on a steady frame of B's shape
@pytest.mark.parametrize("path", ["default", "separate"])
def test_sequence_on_a_steady_frame_of_config_Bs_shape(monkeypatch, path):
    """Six steps with perturbed measurements and varying u, 48 particles x 512 components x 64 measurements, MaxQuantity 600 as
    bench.py sets it: resampling decision and sources and BestParticle exact, particle weights within rtol 1e-6 and every map
    within 1e-7 of orc.slam_update after every step (tests/oracle_parity.py). The first step's corrected lists exceed
    MaxQuantity (asserted on the oracle): the floor is at work."""
    if path == "separate":
        monkeypatch.setenv("PHD_CHAIN_MAX", "0")
    _, C, M, seed = CONFIGS["B"]
    P, maxq = 48, max(600, C)
    f = Frame(P, C, M, seed, weight_profile="steady")
    nav, p = make_nav(f, maxq)
    ne = emitted_counts(p, f, range(P))
    assert np.all(ne > maxq), "the oracle does not exceed MaxQuantity on the first step"
    st = oracle_state(f, 700)
    rng = np.random.default_rng(606)
    nres = 0
    for step in range(6):
        z = f.z + rng.normal(size=f.z.shape) * np.sqrt([2.0, 2.0, 1e-3]) * 0.2 * step
        u = float(rng.uniform(0.05, 0.95))
        best, src, res, _ = orc.slam_update(p, st, z, u=u, threads=THREADS)
        nav.SlamUpdate(None, z, u_resample=u)
        assert_step_matches(nav, st, best, src, res, maxq, "B-shaped steady sequence (%s), step %d" % (path, step))
        nres += int(res)
    assert nres >= 1, "no step resampled"
    nav.close()
