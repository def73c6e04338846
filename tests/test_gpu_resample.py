"""The end of a step — normalise, BestParticle, the depletion test, systematic resampling, the gather of the small arrays and the
rotation of the bank roles (monorfs_amd/csrc/phd_resample.h) — through the C-ABI, against the sequential recurrence of the CPU
oracle: the one-workgroup kernel (its staged path and its walk in global memory) and the four grid kernels. Which of the two
runs is decided by the vector's length and PHD_NR_GRID_MIN, which is read when the handle is made."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import orc
from monorfs_amd.abi import prm3d_defaults
from monorfs_amd.synth import Frame


@pytest.fixture(scope="module")
def nav_mod():
    from monorfs_amd import navigator
    return navigator


def _small_handle(nav_mod):
    """a handle whose own particles do not matter: ResampleParticles / ParticleDepleted take the vector they are given"""
    p = prm3d_defaults(max_particles=4, max_components=600, max_measurements=8)
    return nav_mod.PHDNavigator(p, particlecount=4), p


def _handle(nav_mod, f, maxq=600):
    p = prm3d_defaults(max_particles=f.P, max_components=max(maxq, f.C), max_measurements=max(f.M, 1))
    p.max_quantity = maxq
    nav = nav_mod.PHDNavigator(p, particlecount=f.P)
    nav.upload_state(f.planes(), f.counts, f.poses, f.weights)
    return nav, p


def _resample_vectors(P, rng):
    """exactly uniform (every slot boundary is a tie: the margin test fails and one wave replays the recurrence), random, mostly
    zeros, one particle holding everything, alternating"""
    vectors = {"uniform": np.full(P, 1.0 / P)}
    w = rng.random(P) ** 6
    vectors["random^6"] = w / w.sum()
    w = rng.random(P) * (rng.random(P) < 0.1)
    w[rng.integers(P)] += 1e-3
    vectors["nine tenths zero"] = w / w.sum()
    for at in sorted({0, P // 2, P - 1}):
        w = np.zeros(P)
        w[at] = 1.0
        vectors["all in %d" % at] = w
    w = np.where(np.arange(P) % 2 == 0, 1.0, 1e-12)
    vectors["alternating"] = w / w.sum()
    return vectors


def _check_vectors(nav, p, sizes, rng):
    for P in sizes:
        for name, w in _resample_vectors(P, rng).items():
            for u in (0.0, 2.0 ** -60, 0.5, 1.0 - 2.0 ** -53):
                src, best = nav.ResampleParticles(w, u)
                osrc, obest = orc.resample(w, u)
                assert np.array_equal(src, osrc), "P=%d %s u=%g: %d sources differ" % (P, name, u, np.count_nonzero(src != osrc))
                assert best == obest, "P=%d %s u=%g: best %d, oracle %d" % (P, name, u, best, obest)
            assert nav.ParticleDepleted(w) == orc.particle_depleted(p, w), "P=%d %s" % (P, name)


# The one-workgroup kernel gives every one of its 1024 threads a chunk of ceil(P / 1024) weights and stages the vector in LDS,
# a whole chunk per thread, while that fits beside its static arrays: chunks of up to 17 weights, 17 408 weights. Beyond, it walks
# the slots in global memory.
LARGE_SIZES = [8192, 12345, 16384, 17408, 17409, 18300, 18400, 18432, 20000, 32768]


def large_vector_cases(P):
    """(name, weights, u) of test_resample_large_vectors at one size"""
    rng = np.random.default_rng(P)
    cases = []
    for power, u in ((8, 0.5), (1, 0.25), (30, 0.999999), (2, 1e-12)):
        w = rng.random(P) ** power
        cases.append(("power=%d" % power, w / w.sum(), u))
    cases.append(("uniform", np.full(P, 1.0 / P), 0.5))      # the margin test fails: the fallback on each path
    if P in (16384, 20000):                                  # (the one-wave replay is sequential: the staged and the global branch once each)
        cases.append(("uniform", np.full(P, 1.0 / P), 0.0))
        w = rng.random(P) ** 8
        cases.append(("power=8", w / w.sum(), 0.0))
    return cases


@pytest.mark.parametrize("grid_min", ["0", None], ids=["one-workgroup", "grid"])
@pytest.mark.parametrize("P", LARGE_SIZES)
def test_resample_large_vectors(nav_mod, monkeypatch, P, grid_min):
    """ResampleParticles / ParticleDepleted on the global weight vector of a sharded run (C8: 16 384) and around it, 8192 .. 32 768
    weights, bit-exact against the sequential recurrence on both implementations. PHD_NR_GRID_MIN=0, the one-workgroup kernel:
    chunks of 8 .. 32 weights per thread, the LDS-staged path up to its limit (17 408), the first size beyond it, and the walk in
    global memory. The default: the same sizes on the grid kernels. Besides depleted and flat random vectors: the exactly uniform
    one, on which the margin test fails and one wave replays the recurrence, and u = 0."""
    if grid_min is None:
        monkeypatch.delenv("PHD_NR_GRID_MIN", raising=False)
    else:
        monkeypatch.setenv("PHD_NR_GRID_MIN", grid_min)
    nav, p = _small_handle(nav_mod)
    for name, w, u in large_vector_cases(P):
        src, best = nav.ResampleParticles(w, u)
        osrc, obest = orc.resample(w, u)
        assert np.array_equal(src, osrc), "P=%d %s u=%g: %d sources differ" % (P, name, u, np.count_nonzero(src != osrc))
        assert best == obest, "P=%d %s u=%g: best %d, oracle %d" % (P, name, u, best, obest)
        assert nav.ParticleDepleted(w) == orc.particle_depleted(p, w), "P=%d %s" % (P, name)
    nav.close()


def test_resample_every_launch_shape_and_degenerate_weights(nav_mod):
    """k_normalise_resample decides a particle's slots from prefix sums with an error margin and falls back to the
    recurrence itself (PHDNavigator.cs:724-760) when a boundary is closer than the margin. Sizes around every change of its
    launch shape (256 / 512 / 1024 threads, chunks of 1, 2, ... weights), and weight vectors that sit ON the boundaries
    (exactly uniform: every slot boundary is a tie, the fallback runs), vectors of mostly zeros, one particle holding
    everything, u at both ends of [0, 1): sources and BestParticle bit-exact against the sequential recurrence.
    (8192 and 12 345 weights run on the grid kernels by default.)"""
    nav, p = _small_handle(nav_mod)
    sizes = [1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1000, 1023, 1024, 1025, 4095, 4096, 4097, 8192, 12345]
    _check_vectors(nav, p, sizes, np.random.default_rng(11))
    nav.close()


def test_grid_resampling_at_every_size_and_on_degenerate_weights(nav_mod, monkeypatch):
    """The grid kernels forced on EVERY vector length (PHD_NR_GRID_MIN=1; by default they take 8192 .. 65 536 weights): one
    workgroup and many, lengths around the workgroup and wave boundaries, vectors that sit on the slot boundaries (uniform:
    the margin test fails and one wave replays the recurrence), mostly zeros, one particle holding everything, u at both ends —
    sources and BestParticle bit-exact against the sequential recurrence (PHDNavigator.cs:724-760), the depletion test too."""
    monkeypatch.setenv("PHD_NR_GRID_MIN", "1")
    nav, p = _small_handle(nav_mod)
    sizes = [1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1000, 1024, 1025, 4097, 12345, 16384, 65536]
    _check_vectors(nav, p, sizes, np.random.default_rng(12))
    nav.close()


def test_vectors_beyond_the_grid_take_the_one_workgroup_kernel(nav_mod):
    """65 537 weights and more: the grid's statistics block holds 256 workgroups — the one-workgroup kernel's global-memory walk it is"""
    nav, _ = _small_handle(nav_mod)
    rng = np.random.default_rng(13)
    for P in (65537, 70000):
        w = rng.random(P) ** 8
        w /= w.sum()
        src, best = nav.ResampleParticles(w, 0.37)
        osrc, obest = orc.resample(w, 0.37)
        assert np.array_equal(src, osrc) and best == obest
    nav.close()


@pytest.mark.parametrize("frozen", [False, True])
def test_steps_that_end_on_the_grid_kernels(nav_mod, monkeypatch, frozen):
    """Whole SlamUpdate steps whose end (normalise, BestParticle, depletion, resampling, the gather of the small arrays, the
    rotation of the bank roles) runs on the grid kernels (forced: PHD_NR_GRID_MIN=64) against the oracle and against a handle
    that ends its steps on the one-workgroup kernel: resampling decision, sources and BestParticle exact, weights to the
    tolerance of two summation orders (1e-12 between the kernels, 1e-6 against the oracle), maps bit for bit."""
    f = Frame(300, 50, 12, 520, weight_profile="steady")
    f.weights = np.random.default_rng(5).random(f.P) ** 8     # a depleted set: the first step resamples (the frozen runs repeat that step)
    f.weights /= f.weights.sum()
    one, p = _handle(nav_mod, f)
    monkeypatch.setenv("PHD_NR_GRID_MIN", "64")
    grid, _ = _handle(nav_mod, f)
    st = orc.State(f.P, 700)
    st.poses[:] = f.poses
    st.w[:, :f.C], st.mean[:, :f.C], st.cov[:, :f.C], st.n[:] = f.w, f.mean, f.cov, f.C
    st.weights[:] = f.weights
    rng = np.random.default_rng(521)
    nres = 0
    for step in range(4):
        z = f.z + rng.normal(size=f.z.shape) * np.sqrt([2.0, 2.0, 1e-3]) * 0.3
        u = float(rng.uniform(0.05, 0.95))
        if frozen:          # the frozen step leaves the state where it was: every step starts from the same one, on both handles
            one.set_frozen(True)
            grid.set_frozen(True)
        one.SlamUpdate(None, z, u_resample=u)
        grid.SlamUpdate(None, z, u_resample=u)
        (s1, r1), (s2, r2) = one.resample_sources(), grid.resample_sources()
        assert r1 == r2 and np.array_equal(s1, s2), "step %d: the two kernels resample differently" % step
        assert one.BestParticle == grid.BestParticle
        assert np.allclose(one.VehicleWeights, grid.VehicleWeights, rtol=1e-12, atol=0)
        for i in (0, 17, 150, f.P - 1):
            assert all(np.array_equal(x, y) for x, y in zip(one.MapModel(i), grid.MapModel(i))), "step %d map %d" % (step, i)
        assert np.array_equal(one.poses(), grid.poses())
        if not frozen:
            best, src, res, _ = orc.slam_update(p, st, z, u=u, threads=4)
            assert res == r2 and np.array_equal(src, s2) and best == grid.BestParticle
            assert np.allclose(grid.VehicleWeights, st.weights, rtol=1e-6, atol=1e-300)
        nres += int(r2)
    assert nres >= 1, "no step resampled"
    one.close()
    grid.close()
