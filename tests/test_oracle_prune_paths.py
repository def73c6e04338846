"""The oracle's PruneModel against its second reading, tests/prune_cases.ref_prune, on every family of merge cases: both
state PHDNavigator.cs:913-948 and Gaussian.Merge (Gaussian.cs:297-347) in the reference's order of operations — the oracle
as the reference does, erasing absorbed rows from a list, the second reading with all closeness tests taken first (in
extended precision) and an owner per row —, so the pruned maps must be EQUAL: count, order, and every bit of the weights,
means and covariances. The cases keep every pair 1e-6 away from the threshold, or the two inverses could disagree on one.
Building a case asserts its own conditions (prune_cases.built): that it reaches the path it is for."""
import numpy as np
import pytest

import orc
import prune_cases as pc
from monorfs_amd.abi import prm3d_defaults


def params_for(case):
    p = prm3d_defaults(max_particles=1, max_components=case.capacity, max_measurements=8)
    p.max_quantity, p.min_weight, p.merge_threshold = case.max_quantity, case.min_weight, pc.MERGE_THRESHOLD
    return p


@pytest.mark.parametrize("name", pc.IDS)
def test_oracle_prune_equals_its_second_reading(name):
    case, (rw, rm, rc, info) = pc.built(name)
    ow, om, oc = orc.prune(params_for(case), case.mix())
    assert len(ow) == len(rw) == info.cut - len(info.absorbed)
    assert np.array_equal(ow, rw), "weights / order: first difference at %d" % int(np.flatnonzero(ow != rw)[0])
    assert np.array_equal(om, rm), "means: first difference at row %d" % int(np.flatnonzero((om != rm).any(axis=1))[0])
    assert np.array_equal(oc, rc), "covariances: first difference at row %d" % int(np.flatnonzero((oc != rc).any(axis=(1, 2)))[0])


@pytest.mark.parametrize("name", pc.ORDER_IDS)
def test_order_cases_reach_their_branch_of_phase_a(name):
    """the maps that take the sort half of prune_merge_body down each of its branches (tests/test_gpu_prune_paths.py runs them on
    the device): the branch is predicted from the weights alone, and nothing in such a map merges"""
    case, branch, deciders = pc.order_case(name)
    assert pc.order_branch(case.w, case.max_quantity, case.min_weight)[0] == branch
    assert deciders <= pc.run_deciders(case.w, case.max_quantity, case.min_weight)
    ow, om, oc = orc.prune(params_for(case), case.mix())
    order = np.argsort(-case.w, kind="stable")[:min(case.max_quantity, len(case.w))]
    assert np.array_equal(ow, case.w[order]) and np.allclose(om, case.mean[order], rtol=1e-15, atol=0)   # (Merge of one row: w m / w)


def test_second_reading_on_a_hand_made_map():
    """three rows on a line, by hand: the heaviest takes the middle one; the lightest is outside the heaviest's distance and
    inside the middle row's (a covariance of 1), which is absorbed and so never asks: two rows out, the merged one with the
    moments Gaussian.Merge gives"""
    w = np.array([0.2, 1.0, 0.5])
    mean = np.array([[0.05, 0, 0], [0.0, 0, 0], [0.02, 0, 0]])
    cov = np.array([np.eye(3) * 1e-2, np.eye(3) * 1e-2, np.eye(3) * 1.0])
    ow, om, oc, info = pc.ref_prune(w, mean, cov, 1e-3, 600, 0.3)
    assert list(info.order) == [1, 2, 0] and list(info.owner) == [-1, 0, -1] and info.skipped == 0
    assert list(info.nclose) == [1, 1, 0]          # the middle row (rank 1) is close to the last under its covariance of 1
    W = 1.5
    assert ow[0] == W and ow[1] == 0.2
    assert np.allclose(om[0], [0.5 * 0.02 / W, 0, 0], rtol=1e-15)
    second = (1.0 * 1e-2 + 0.5 * (1.0 + 0.02 ** 2)) / W - om[0][0] ** 2
    assert np.isclose(oc[0][0, 0], second, rtol=1e-14) and np.isclose(oc[0][1, 1], (1e-2 + 0.5) / W, rtol=1e-14)
    assert np.isclose(info.margin, abs(0.02 ** 2 / 1e-2 - 0.09) / 0.09, rtol=1e-12)   # the nearest to the threshold: 0.04 against 0.09
