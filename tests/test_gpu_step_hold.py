"""phd_step_hold_async on the device: a mapping-only step that one particle slot sits out, at every launch shape a step has
(one launch per particle chain with and without helper workgroups, separate kernels, two streams), behind a step that
resampled, posted back to back, and what it refuses. Everything is compared bit for bit: the held slot with its own state in
front of the step, every other slot with the plain step's result on a second handle."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from monorfs_amd.abi import PHD_ERR_BAD_ARGUMENT, prm3d_defaults
from monorfs_amd.synth import Frame

CAP, M, CMAX = 64, 8, 30      # max_components, measurements, the largest uploaded map
SHAPES = [1, 2, 257, 513, 1024]   # smallest | past PHD_DSPLIT_MAX | past PHD_CHAIN_MAX: separate kernels | two streams


def params(P, min_effective_particle=None):
    p = prm3d_defaults(max_particles=P, max_components=CAP, max_measurements=M)
    p.max_quantity = 40           # the `filter` set of tests/paramspace.py
    if min_effective_particle is not None:
        p.min_effective_particle = min_effective_particle
    return p


def handle(P, **more):
    from monorfs_amd import navigator
    return navigator.PHDNavigator(params(P, **more), particlecount=P)


_frames = {}


def frame(P):
    """random maps of 5 - 30 components per particle, one pose and one measurement set (made once per particle count)"""
    if P not in _frames:
        f = Frame(P, CMAX, M, 7000 + P, weight_profile="steady")
        rng = np.random.default_rng(7100 + P)
        f.counts = rng.integers(5, CMAX + 1, P).astype(np.int32)
        planes = f.planes(CAP)
        for i in range(P):
            planes[:, i, f.counts[i]:] = 0
        _frames[P] = (f, planes)
    return _frames[P]


def loaded(P, **more):
    f, planes = frame(P)
    nav = handle(P, **more)
    nav.upload_state(planes, f.counts, f.poses, f.weights)
    nav.set_measurements(f.z)
    return nav


def state(nav):
    nav.sync()
    return nav.download_state(CAP)


def plain_step(nav):
    nav.OnlyMapping = True
    nav.step_async()


def same(a, b, slots=slice(None)):
    """count, records, pose and weight of the slots, bit for bit"""
    return (np.array_equal(a[1][slots], b[1][slots]) and np.array_equal(a[0][:, slots], b[0][:, slots])
            and np.array_equal(a[2][slots], b[2][slots]) and np.array_equal(a[3][slots], b[3][slots]))


def check_hold(before, held_state, plain_state, h, P):
    others = np.arange(P) != h
    assert same(held_state, before, [h]), "the held slot is not what it was in front of the step"
    assert same(held_state, plain_state, others), "a slot that was not held differs from the plain step's"
    assert not (np.array_equal(plain_state[1][h], before[1][h]) and np.array_equal(plain_state[0][:, h], before[0][:, h])), \
        "the plain step left the slot as it was: the case shows nothing"


@pytest.mark.parametrize("P", SHAPES)
def test_hold_against_plain_step(P):
    b = loaded(P)
    before = state(b)
    plain_step(b)
    plain = state(b)
    b.close()
    for h in sorted({0, P - 1, P // 2}):
        a = loaded(P)
        assert same(state(a), before)
        a.StepHold(h)
        check_hold(before, state(a), plain, h, P)
        a.close()


@pytest.mark.parametrize("P", [2, 513, 1024])
def test_hold_nobody_is_the_plain_step(P):
    a, b = loaded(P), loaded(P)
    a.StepHold(-1)
    plain_step(b)
    got, want = state(a), state(b)
    assert same(got, want)
    assert not np.array_equal(got[0], frame(P)[1])
    a.close(), b.close()


@pytest.mark.parametrize("P", [2, 513, 1024])
def test_hold_behind_a_resampling_step(P):
    """a SLAM step that resamples (sources not the identity: the mixtures of the new state sit behind an indirection in another
    bank than its small arrays), the held step right behind it without a sync"""
    f, _ = frame(P)
    weights = np.full(P, 1e-6)
    weights[P - 1] = 1.0          # one heavy particle, the last: the effective count is about 1 and slot 0 is copied from it
    weights /= weights.sum()
    h = P // 2

    def slam(nav):
        nav.set_weights(weights)
        nav.OnlyMapping = False
        nav.step_async(0.37)

    # (MinEffectiveParticle 0.9: two particles have an effective count of at least 1, which the default 0.1 never calls depleted)
    loaded_ = lambda: loaded(P, min_effective_particle=0.9)
    c = loaded_()                 # the state in front of the held step, from a handle that stops there
    slam(c)
    before = state(c)
    src, resampled = c.resample_sources()
    assert resampled and not np.array_equal(src, np.arange(P)), "the SLAM step did not resample away from the identity"
    c.close()
    a, b = loaded_(), loaded_()
    slam(a)
    a.StepHold(h)
    slam(b)
    plain_step(b)
    check_hold(before, state(a), state(b), h, P)
    a.close(), b.close()


@pytest.mark.parametrize("P", [3, 1024])
def test_held_steps_posted_back_to_back(P):
    f, _ = frame(P)
    rng = np.random.default_rng(7200 + P)
    held = [0, P - 1, -1, P // 2]
    frames = [(f.poses + rng.normal(0, 1e-3, f.poses.shape) * [1, 1, 1, 0, 0, 0, 0], f.z + rng.normal(0, 1, f.z.shape) * [0.5, 0.5, 0.01]) for _ in held]
    a, b = loaded(P), loaded(P)
    for h, (poses, z) in zip(held, frames):
        a.set_poses(poses)
        a.set_measurements(z)
        a.StepHold(h)
    for h, (poses, z) in zip(held, frames):
        b.set_poses(poses)
        b.sync()
        b.set_measurements(z)
        b.sync()
        b.StepHold(h)
        b.sync()
    # ... and with nothing at all between them: from 1024 particles the plain steps among these are not forked and joined
    tail = [1, -1, -1, P - 1, 0]
    for h in tail:
        a.StepHold(h)
    for h in tail:
        b.StepHold(h)
        b.sync()
    got, want = state(a), state(b)
    assert same(got, want)
    assert not np.array_equal(got[0], frame(P)[1])
    a.close(), b.close()


def refused(nav, held):
    from monorfs_amd.navigator import PHDError
    before = state(nav)
    with pytest.raises(PHDError) as e:
        nav.StepHold(held)
    assert e.value.status == PHD_ERR_BAD_ARGUMENT
    assert same(state(nav), before)


def test_refusals_leave_the_state():
    P = 3
    a = loaded(P)
    refused(a, P)
    refused(a, -2)
    a.set_frozen(True)
    refused(a, 1)
    a.set_frozen(False)
    before = state(a)
    a.StepHold(1)                 # (and it still steps)
    after = state(a)
    assert same(after, before, [1]) and not np.array_equal(after[0], before[0])
    a.close()


def test_a_handle_without_particles_is_refused():
    from monorfs_amd import _lib
    lib = _lib.load()
    p = params(3)
    h = lib.phd_create(C.byref(p), 0)
    assert h, lib.phd_create_error()
    try:
        assert lib.phd_particle_count(h) == 0
        for held in (-1, 0):
            assert lib.phd_step_hold_async(h, held) == PHD_ERR_BAD_ARGUMENT
        assert lib.phd_sync(h) == 0 and lib.phd_particle_count(h) == 0
    finally:
        lib.phd_destroy(h)


def test_a_multi_device_handle_is_refused():
    from monorfs_amd import navigator
    from monorfs_amd.navigator import PHDError
    f, planes = frame(2)
    try:
        nav = navigator.PHDNavigator(params(2), particlecount=2, devices=[0, 0])
    except PHDError:
        pytest.skip("phd_create_multi does not take the same device twice here")
    nav.upload_state(planes, f.counts, f.poses, f.weights)
    nav.set_measurements(f.z)
    before = nav.download_state(CAP)
    for held in (-1, 0):
        with pytest.raises(PHDError) as e:
            nav.StepHold(held)
        assert e.value.status == PHD_ERR_BAD_ARGUMENT
    assert same(nav.download_state(CAP), before)
    nav.close()
