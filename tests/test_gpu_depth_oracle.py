"""Whole Kinect steps against the CPU oracle: an occluding depth map with NaN holes, a different one in every step, set on
the device (phd_set_depth_map) and in the oracle (orc.depth_map) alike; three SlamUpdates with varying u and perturbed
measurements, every particle after every step (tests/oracle_parity.py: resampling flag, sources and BestParticle exact,
weights 1e-6, every map 1e-7, OSPA of the best map 1e-4). One test id per code path of the DEPTH instantiation of the step:
the one-launch chain with and without its helper workgroups and with the step's end folded in, the separate kernels with
the fused and the unfused emit + prune, the timed mode and the multi-device handle. The switches are read at phd_create."""
import os

import numpy as np
import pytest

import kinect_ref
import orc
from monorfs_amd.abi import prm3d_defaults
from monorfs_amd.synth import CONFIGS, Frame
from oracle_parity import assert_step_matches, oracle_state

pytestmark = pytest.mark.gpu

W, H = 640, 480
THREADS = min(16, os.cpu_count() or 1)   # (a command on the GPU machines gets 16 CPUs; os.cpu_count() shows the whole box)
SHAPES = dict(CONFIGS, S512=(512, 1024, 128, 1004))   # S's components and measurements on 512 particles: the chain's size


def frame(cfg):
    P, C, M, seed = SHAPES[cfg]
    f = Frame(P, C, M, seed, weight_profile="steady")
    f.z[:, 2] = np.maximum(f.z[:, 2], 0.25)   # (out of the near range ramp, as tests/test_gpu_depth_map.py)
    return f


def make(f, devices=None):
    from monorfs_amd import navigator
    maxq = max(600, f.C)
    p = prm3d_defaults(max_particles=f.P, max_components=maxq, max_measurements=f.M)
    p.max_quantity = maxq
    nav = navigator.PHDNavigator(p, particlecount=f.P, devices=devices)
    nav.upload_state(f.planes(), f.counts, f.poses, f.weights)
    return nav, p


def occluder(seed):
    return kinect_ref.occluding_map(np.random.default_rng(seed), W, H, near=0.8, far=2.0, blocks=(8, 6), holes=0.05)


def steps(f, seed):
    """three (measurements, u, depth map) triples: perturbed z (kept out of the near ramp), varying u, a map per step"""
    rng = np.random.default_rng(seed)
    out = []
    for s in range(3):
        z = f.z + rng.normal(size=f.z.shape) * np.sqrt([2.0, 2.0, 1e-3]) * 0.2 * s
        z[:, 2] = np.maximum(z[:, 2], 0.25)
        out.append((z, float(rng.uniform(0.05, 0.95)), occluder(seed + 10 * s)))
    return out


def assert_the_map_bites(p, st, z, depth, what, sample=8):
    """no vacuous pass: on the predicted components of a sample of particles, the map moves at least 20 % of the PDs, sets
    some to 0 and puts some strictly between 0 and the PD without the map (the depth ramp)"""
    moved = zero = ramp = total = 0
    for i in np.linspace(0, st.P - 1, sample).astype(int):
        pw, pm, _ = orc.predict(p, st.poses[i], z, st.map(i))
        zh = np.array([orc.measure_perfect(p, st.poses[i], m) for m in pm])
        pd0 = orc.detection_probability_m(p, zh)
        with orc.depth_map(depth):
            pd = orc.detection_probability_m(p, zh)
        moved += np.count_nonzero(pd != pd0)
        zero += np.count_nonzero((pd == 0) & (pd0 > 0))
        ramp += np.count_nonzero((pd > 0) & (pd < pd0))
        total += len(pd)
    assert moved >= 0.2 * total, "%s: the map moved the PD of %d of %d predicted components only" % (what, moved, total)
    assert zero > 0 and ramp > 0, "%s: %d components at PD 0, %d on the depth ramp" % (what, zero, ramp)


# id: (shape, environment at phd_create, timed, devices)
PATHS = {
    "chain_helpers_A24": ("A24", {}, False, None),
    "chain_helpers_A": ("A", {}, False, None),
    "chain_no_helpers_A": ("A", {"PHD_DSPLIT_MAX": "0"}, False, None),
    "chain_no_helpers_B512": ("B512", {}, False, None),
    "separate_fused_emit_prune_B1024": ("B1024", {}, False, None),
    "separate_unfused_B1024": ("B1024", {"PHD_FUSE_EP": "0"}, False, None),
    "separate_unfused_S512": ("S512", {"PHD_CHAIN_MAX": "0"}, False, None),
    "timed_A": ("A", {}, True, None),
    "timed_B1024": ("B1024", {}, True, None),
    "multi_device_A": ("A", {}, False, [0, 0]),
}


@pytest.mark.parametrize("path", list(PATHS))
def test_kinect_steps_against_the_oracle(monkeypatch, path):
    """Cost, measured on one MI355X box with the oracle on 16 threads: the ids (eleven when this was measured, ten now) took 8.5 s together, almost all of
    it the oracle's host time — S512 2.4 s, each B1024 id 1.5 s, B512 0.8 s, each A-sized id 0.1 - 0.3 s; the device's
    steps are a few milliseconds of that."""
    cfg, env, timed, devices = PATHS[path]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    f = frame(cfg)
    nav, p = make(f, devices)
    if timed:   # (each step reads the same state and leaves it: the oracle runs every step from the start too)
        nav.set_frozen(True)
        nav.set_all_pairs(True)
    st0 = oracle_state(f, p.max_quantity)
    st = st0
    nres = 0
    for s, (z, u, depth) in enumerate(steps(f, 700 + 31 * list(PATHS).index(path))):
        what = "%s step %d" % (path, s)
        if timed:
            st = st0.copy()
        assert_the_map_bites(p, st, z, depth, what)
        with orc.depth_map(depth):
            best, src, res, _ = orc.slam_update(p, st, z, u=u, threads=THREADS)
        nav.set_depth_map(depth)
        nav.SlamUpdate(None, z, u_resample=u)
        assert_step_matches(nav, st, best, src, res, p.max_quantity, what, bulk=not timed)
        nres += int(res)
    if cfg == "S512":   # (S's frame: every WeightAlpha of the first step underflows to 0 — on both sides, asserted above — so the
        assert np.all(st.weights == 0)   # weights stay 0 and nothing can resample; tests/test_full_size.py says the same at S)
    else:
        assert nres >= 1, "%s: no step resampled" % path
    nav.close()
