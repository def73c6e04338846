"""The merge half of prune_merge_body (monorfs_amd/csrc/phd_prune.h: the slab, the grid and its hash, the pair search, the
resolving wave, the moment match) path by path, in each of the three launches that contain the body: k_particle_chain (the
default for a small particle set), k_prune_merge and k_emit_prune (the separate kernels, PHD_CHAIN_MAX=0 with PHD_FUSE_EP
0 / 1; the switches are read when the handle is made). Which launch ran is read off the kernel timers of the very run whose
result is compared. At one measurement block the chain's LDS pool is the prune's own layout plus a few words, so it fits for
every MaxQuantity phd_create admits: the default IS the chain in every case here, and the assertion says so.

The cases are those of tests/prune_cases.py — each names the path it is for and has proved, from its plain reference, that it
reaches it. A case goes through the boundary as the prior map of one Linear2D particle far outside the visible square:
every detection probability is 0, the correction passes the map on unchanged (asserted), and PruneModel sees exactly the
case. PruneModel's input is then bit-equal to the oracle's, so the comparison with orc.prune is held to what
test_gpu_round2.test_far_from_the_origin_stage_by_stage holds it to in that situation: count and order exact, weights
1e-12, means 1e-13, the covariances' upper triangle 1e-9 (+ 1e-16).

The sort half (phase A, prune_order) goes the same way: prune_cases.order_case has the smallest map for each of its branches
— register sort, ranked with and without reload rounds, the one-pass fallback, the passes with and without refill —, means
far apart so that the output is the sorted cut itself; the branch is predicted from the weights in numpy and asserted.

The pass-through reads every record from the prior bank: the emitted records and the patched births are the last test's,
a PRM3D frame whose detection updates and births merge, against orc.prune(orc.correct(orc.predict())) at the stage
tolerance 1e-7."""
import json
import os

import numpy as np
import pytest

import orc
import prune_cases as pc
from monorfs_amd.abi import params_from_dict, prm3d_defaults
from monorfs_amd.synth import Frame
from test_gpu_parity import assert_mix_close

pytestmark = pytest.mark.gpu

KAT = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "phdnavigator_kat.json")))
IU = np.triu_indices(3)

LAUNCHES = {   # id -> (environment, what a stage run without alpha launches per particle range)
    "chain": ({}, {"k_particle_chain": 1}),
    "prune_merge": ({"PHD_CHAIN_MAX": "0", "PHD_FUSE_EP": "0"}, {"k_sweep": 1, "k_emit_finish": 1, "k_prune_merge": 1}),
    "emit_prune": ({"PHD_CHAIN_MAX": "0", "PHD_FUSE_EP": "1"}, {"k_sweep": 1, "k_emit_prune": 1}),
}


@pytest.fixture(scope="module")
def nav_mod():
    from monorfs_amd import navigator
    return navigator


def select_launch(monkeypatch, launch):
    for name in ("PHD_CHAIN_MAX", "PHD_FUSE_EP"):
        monkeypatch.delenv(name, raising=False)
    for name, value in LAUNCHES[launch][0].items():
        monkeypatch.setenv(name, value)


def timed_stage_run(nav, z, launch, what):
    """one stage run with the kernel timers on: the kernels it launched are the ones the id names"""
    nav.timing_reset(True)
    nav.run_stages(z, with_alpha=False)
    ran = nav.last_timing_counts()
    nav.timing_reset(False)
    assert ran == LAUNCHES[launch][1], "%s: the stage run launched %r, the id says %r" % (what, ran, LAUNCHES[launch][1])


def prune_through_the_device(nav_mod, case, launch, what):
    """PruneModel of a prune_cases.Case on the device (tests/test_gpu_round4.prune_through_the_device with the means and
    covariances of the case): the case is the prior map of a Linear2D particle 140 km from it, so the correction step hands
    it on unchanged — asserted, record by record — and no measurement is given."""
    params = dict(KAT["params"], max_quantity=case.max_quantity, min_weight=case.min_weight, merge_threshold=pc.MERGE_THRESHOLD)
    p = params_from_dict(params, max_particles=1, max_components=case.capacity, max_measurements=8)
    pose = np.array([100000.0, -100000.0, 0, 1.0, 0, 0, 0])
    nav = nav_mod.PHDNavigator(p, particlecount=1, pose=pose)
    try:
        nav.reset(pose, case.mix(), 1)
        timed_stage_run(nav, np.zeros((0, 3)), launch, what)
        cw, cm, cc = nav.CorrectConditional(0)
        assert len(cw) == len(case.w), "%s: the correction step kept %d of %d components" % (what, len(cw), len(case.w))
        # (by weight, bit-equal weights by their means: the corrected list is in no particular order)
        a, b = np.lexsort((cm[:, 2], cm[:, 1], cm[:, 0], cw)), np.lexsort((case.mean[:, 2], case.mean[:, 1], case.mean[:, 0], case.w))
        assert np.array_equal(cw[a], case.w[b]) and np.array_equal(cm[a], case.mean[b]) and \
            np.array_equal(cc[a][:, IU[0], IU[1]], case.cov[b][:, IU[0], IU[1]]), "%s: the correction step did not pass the map on unchanged" % what
        got = nav.PruneModel(0)
    finally:
        nav.close()
    return p, got


def relative(got, want):
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300))) if want.size else 0.0


@pytest.mark.parametrize("launch", list(LAUNCHES))
@pytest.mark.parametrize("name", pc.IDS)
def test_merge_paths_against_the_oracle(nav_mod, monkeypatch, name, launch):
    what = "%s through %s" % (name, launch)
    case, (rw, rm, rc, info) = pc.built(name)
    select_launch(monkeypatch, launch)
    p, got = prune_through_the_device(nav_mod, case, launch, what)
    want = orc.prune(p, case.mix())
    assert len(want[0]) == len(rw) and np.array_equal(want[0], rw)      # (the oracle and its second reading: the same map)
    print("%s: cut %d, absorbed %d, device %d rows, oracle %d" % (what, info.cut, len(info.absorbed), len(got[0]), len(want[0])))
    assert len(got[0]) == len(want[0]), "%s: %d rows, the oracle has %d (a cut of %d rows, %d of them absorbed)" % (
        what, len(got[0]), len(want[0]), info.cut, len(info.absorbed))
    print("%s: largest relative difference: weights %.3g, means %.3g, covariances %.3g" % (
        what, relative(got[0], want[0]), relative(got[1], want[1]), relative(got[2][:, IU[0], IU[1]], want[2][:, IU[0], IU[1]])))
    assert np.allclose(got[0], want[0], rtol=1e-12, atol=0), "%s: weights / order, first at row %d" % (
        what, int(np.flatnonzero(~np.isclose(got[0], want[0], rtol=1e-12, atol=0))[0]))
    assert np.allclose(got[1], want[1], rtol=1e-13, atol=0), "%s: means (largest relative difference %g)" % (what, relative(got[1], want[1]))
    assert np.allclose(got[2][:, IU[0], IU[1]], want[2][:, IU[0], IU[1]], rtol=1e-9, atol=1e-16), "%s: covariances" % what


# ---- the sort half: every branch of phase A (prune_order), at the smallest size that reaches it ---------------------------------------
@pytest.mark.parametrize("launch", list(LAUNCHES))
@pytest.mark.parametrize("name", pc.ORDER_IDS)
def test_order_branches_against_the_oracle(nav_mod, monkeypatch, name, launch):
    """Means far apart, so nothing merges and PruneModel's output is the sorted cut itself: count and order exact against
    orc.prune, the weights bit-equal. Which branch a case takes — and, on the sorting branches, that neighbours among the kept
    rows are told apart by the 32 weight bits in LDS, by the full weight and by the canonical index — is predicted from its
    weights in numpy (prune_cases.order_branch, run_deciders) and asserted; the device is not asked."""
    what = "%s through %s" % (name, launch)
    case, branch, deciders = pc.order_case(name)
    took = pc.order_branch(case.w, case.max_quantity, case.min_weight)
    print("%s: %d weights, MaxQuantity %d: branch %s (sort width %d), run deciders %s" % (
        what, len(case.w), case.max_quantity, took[0], took[2], sorted(pc.run_deciders(case.w, case.max_quantity, case.min_weight))))
    assert took[0] == branch and deciders <= pc.run_deciders(case.w, case.max_quantity, case.min_weight)
    select_launch(monkeypatch, launch)
    p, got = prune_through_the_device(nav_mod, case, launch, what)
    want = orc.prune(p, case.mix())
    assert len(got[0]) == len(want[0]) == min(len(case.w), case.max_quantity)
    assert np.array_equal(got[0], want[0]), "%s: weights / order, first difference at row %d" % (what, int(np.flatnonzero(got[0] != want[0])[0]))
    assert np.allclose(got[1], want[1], rtol=1e-13, atol=0), "%s: means / order, first difference at row %d" % (
        what, int(np.flatnonzero(~np.isclose(got[1], want[1], rtol=1e-13, atol=0).all(axis=1))[0]))


# ---- rows that do not come from the prior bank: detection updates (emit_rec) and births (patched) ---------------------------------
def packed_frame(seed):
    """2 particles, 16 measurements, 64 components in 16 groups of four neighbours a few millimetres apart: a measurement
    that detects a group moves its four components onto nearly one point, and their detection updates merge; a measurement
    in unexplored space leaves a birth whose own detection update takes its misdetection copy"""
    f = Frame(2, 16, 16, seed, weight_profile="steady")
    f.z[:, 2] = np.maximum(f.z[:, 2], 0.25)
    rng = np.random.default_rng([seed, 1])
    f.mean = np.repeat(f.mean, 4, axis=1) + rng.normal(size=(f.P, 64, 3)) * 4e-3
    f.cov = np.repeat(np.array(f.cov), 4, axis=1)
    f.w = np.repeat(np.array(f.w), 4, axis=1) * rng.uniform(0.5, 1.0, (1, 64))
    f.C = 64
    f.counts = np.full(f.P, 64, np.int32)
    return f


PACKED_SEED = 3


@pytest.mark.parametrize("launch", list(LAUNCHES))
def test_detection_updates_and_births_merge(nav_mod, monkeypatch, launch):
    what = "packed frame through %s" % launch
    f = packed_frame(PACKED_SEED)
    p = prm3d_defaults(max_particles=f.P, max_components=600, max_measurements=f.M)
    want = []
    for i in range(f.P):
        pred = orc.predict(p, f.poses[i], f.z, f.map(i))
        cor = orc.correct(p, f.poses[i], f.z, pred)
        pr = orc.prune(p, cor)
        info = pc.ref_prune(cor[0], cor[1], cor[2], p.min_weight, p.max_quantity, p.merge_threshold)[3]
        assert len(pr[0]) == info.cut - len(info.absorbed)
        # where the rows of the merged sets come from, by canonical index: prior copies, births' copies, detection updates
        origin = info.order[np.concatenate([info.absorbed, np.unique(info.owner[info.absorbed])])]
        births, updates = np.count_nonzero((origin >= f.C) & (origin < len(pred[0]))), np.count_nonzero(origin >= len(pred[0]))
        print("%s, particle %d: %d corrected, cut %d, %d absorbed, in merged sets %d births and %d detection updates, margin %.2e" % (
            what, i, len(cor[0]), info.cut, len(info.absorbed), births, updates, info.margin))
        assert len(info.absorbed) >= 10 and births >= 1 and updates >= 1
        assert info.margin >= 1e-5
        want.append(pr)
    select_launch(monkeypatch, launch)
    nav = nav_mod.PHDNavigator(p, particlecount=f.P)
    try:
        nav.upload_state(f.planes(f.C), f.counts, f.poses, f.weights)
        timed_stage_run(nav, f.z, launch, what)
        for i in range(f.P):
            assert_mix_close(nav.PruneModel(i), want[i], 1e-7, "%s: prune[%d]" % (what, i))
    finally:
        nav.close()
