"""Device steps against the CPU oracle (tests/orc.py) at the edges of the launch shapes phdhip.hip picks from a frame:
the measurement blocks of zb_of(M) (1, 2 or 4 blocks of 64 lanes; the HALF layout up to 32 measurements), the DEPTH build
of a step with a depth map, the one-launch chain against the separate kernels (emit + prune fused or not), the timed mode
and the two-stream step; inside the kernels the prior-component tiles of the sweep (128 components), its compact birth
sums (at most SW_UMAX = 16 open measurements), the landmark arrays of k_alpha_assoc (LDS up to ALPHA_JL = 256 landmarks,
an HBM slab up to Jcap = min(1024, max_quantity rounded up to 64), PHD_ERR_CAPACITY beyond) and the bound of the quasi
set log-likelihood's landmark set.

Every id names the path the launch code's own rule gives its frame — the class (zb_of(M); M <= 32: HALF), the depth map
(DEPTH) and the kernels — and proves it: one more step on the same handle, with the same measurement count, depth state
and environment, outside the compared steps, with the kernel timers on, must report exactly that path's kernels. Up to
chain_max particles the path is the chain: at max_quantity 600 and 1100 its LDS fits every class (phd_create, chain_ok).
Tolerances as in tests/test_gpu_parity.py (stages) and tests/oracle_parity.py (whole steps)."""
import concurrent.futures
import os

import numpy as np
import pytest

import orc
from monorfs_amd.abi import PHD_ERR_BAD_ARGUMENT, PHD_ERR_CAPACITY, prm3d_defaults
from monorfs_amd.synth import Frame, measure_perfect_identity, measure_to_map_identity
from oracle_parity import assert_step_matches, oracle_state
from test_gpu_depth_oracle import assert_the_map_bites, occluder
from test_gpu_parity import assert_mix_close, match_unordered

pytestmark = pytest.mark.gpu

THREADS = min(16, os.cpu_count() or 1)   # (a command on the GPU machines gets 16 CPUs; os.cpu_count() shows the whole box)

KERNELS = {   # what launch_map launches per sub-range, by path
    "chain": {"k_particle_chain"},
    "separate-fused": {"k_sweep", "k_emit_prune", "k_alpha_assoc", "k_alpha_density"},
    "separate-unfused": {"k_sweep", "k_emit_finish", "k_prune_merge", "k_alpha_assoc", "k_alpha_density"},
}


def zb_of(M):
    return 1 if M <= 64 else (2 if M <= 128 else 4)


def klass(M):
    """the measurement-block class of launch_map: HALF (one block, two components per visit), ZB1, ZB2, ZB4"""
    return "half" if M <= 32 else "zb%d" % zb_of(M)


def path_of(P, M, env):
    """the launch code's rule: the chain up to chain_max particles (PHD_CHAIN_MAX, default 512), else the separate kernels
    with k_emit_finish + k_prune_merge fused into k_emit_prune for one measurement block unless PHD_FUSE_EP forces it"""
    if P <= int(env.get("PHD_CHAIN_MAX", 512)):
        return "chain"
    fuse = env.get("PHD_FUSE_EP")
    fused = zb_of(M) == 1 if fuse is None else fuse != "0"
    return "separate-fused" if fused else "separate-unfused"


def launches(path, streams=1):
    """{kernel: launches} of one step on `path` with `streams` particle sub-ranges"""
    want = {k: streams for k in KERNELS[path]}
    want["k_normalise_resample"] = 1
    return want


def assert_path(nav, steps, want, what):
    """one more step per (measurements, depth map) of `steps` on the handle with the kernel timers on: the kernels they
    launched and how often, against `want`"""
    nav.timing_reset(True)
    for z, depth in steps:
        nav.set_depth_map(depth)
        nav.SlamUpdate(None, z, u_resample=0.5)
    got = nav.last_timing_counts()
    nav.timing_reset(False)
    assert got == want, "%s: the timed step launched %r, the path in the id is %r" % (what, got, want)


def frame(P, C, M, seed):
    """synth.Frame (clutter tops up what the map's detections do not give), the measurements kept out of the near range
    ramp (as tests/test_gpu_depth_oracle.py); C = 0: an empty map"""
    f = Frame(P, max(C, 1), M, seed, weight_profile="steady")
    f.z[:, 2] = np.maximum(f.z[:, 2], 0.25)
    if C == 0:
        f.C = 0
        f.counts[:] = 0
        f.w, f.mean, f.cov = f.w[:, :0], f.mean[:, :0], f.cov[:, :0]
    return f


def make(f, maxq=600, max_measurements=None, pd=None, emit_capacity=0):
    from monorfs_amd import navigator
    mm = max(f.M, 1) if max_measurements is None else max_measurements
    p = prm3d_defaults(max_particles=f.P, max_components=max(maxq, f.C), max_measurements=mm)
    p.max_quantity = maxq
    p.emit_capacity = emit_capacity
    if pd is not None:
        p.pd = pd
    nav = navigator.PHDNavigator(p, particlecount=f.P)
    upload(nav, f)
    return nav, p


def upload(nav, f):
    nav.upload_state(f.planes(max(f.C, 1)), f.counts, f.poses, f.weights)


def oracle_stages(p, f, z, i):
    pred = orc.predict(p, f.poses[i], z, f.map(i))
    cor = orc.correct(p, f.poses[i], z, pred)
    pr = orc.prune(p, cor)
    a, sll = orc.weight_alpha(p, f.poses[i], z, pred, pr)
    return pred, cor, pr, a, sll


def stage_parity(nav, p, f, z, depth=None, stride=1):
    """the stages of one step on every particle (every stride-th; the oracle's on THREADS host threads): the predicted and
    pruned mixtures in order, the corrected one as a set, set log-likelihood and alpha. Returns the oracle's results."""
    nav.set_depth_map(depth)
    nav.run_stages(z, with_alpha=True)
    alpha, setll = nav.WeightAlpha(), nav.SetLogLikelihood()
    with orc.depth_map(depth):
        with concurrent.futures.ThreadPoolExecutor(THREADS) as ex:
            want = list(ex.map(lambda i: oracle_stages(p, f, z, i), range(0, f.P, stride)))
    for i, (pred, cor, pr, a, sll) in zip(range(0, f.P, stride), want):
        assert_mix_close(nav.PredictConditional(i), pred, 1e-9, "predict[%d]" % i)
        keep = ~(cor[0] < p.min_weight)
        match_unordered(nav.CorrectConditional(i), tuple(x[keep] for x in cor), 1e-9)
        assert_mix_close(nav.PruneModel(i), pr, 1e-7, "prune[%d]" % i)
        assert np.isclose(setll[i], sll, rtol=1e-9, atol=1e-9), "set log-likelihood[%d]: %r vs %r" % (i, setll[i], sll)
        assert np.isclose(alpha[i], a, rtol=1e-6, atol=0), "alpha[%d]: %r vs %r" % (i, alpha[i], a)
    return want


def perturbed(z, rng, scale=0.2):
    z = z + rng.normal(size=z.shape) * np.sqrt([2.0, 2.0, 1e-3]) * scale
    z[:, 2] = np.maximum(z[:, 2], 0.25)
    return z


def biting_map(p, st, z, seed, what):
    """an occluding map that moves at least 20 % of the predicted PDs, some to 0 and some onto the depth ramp
    (tests/test_gpu_depth_oracle.py): the first of a few seeds"""
    for k in range(4):
        d = occluder(seed + 7919 * k)
        try:
            assert_the_map_bites(p, st, z, d, what)
            return d
        except AssertionError:
            if k == 3:
                raise


def whole_steps(nav, p, f, seed, depth, timed, what, nsteps=3):
    """three SlamUpdates from the uploaded state (perturbed measurements, varying u, a fresh occluding map per step where
    `depth`), every particle after every step against the oracle; a frozen handle (timed) steps from the same state.
    Returns the last step's map."""
    rng = np.random.default_rng(seed)
    st0 = oracle_state(f, p.max_quantity)
    st = st0
    dmap = None
    for s in range(nsteps):
        z = perturbed(f.z, rng, 0.2 * s)
        u = float(rng.uniform(0.05, 0.95))
        w = "%s step %d" % (what, s)
        if timed:
            st = st0.copy()
        dmap = biting_map(p, st, z, seed + 10 * s, w) if depth else None
        with orc.depth_map(dmap):
            best, src, res, _ = orc.slam_update(p, st, z, u=u, threads=THREADS)
        nav.set_depth_map(dmap)
        nav.SlamUpdate(None, z, u_resample=u)
        assert_step_matches(nav, st, best, src, res, p.max_quantity, w, bulk=not timed)
    return dmap


# ---- 1. measurement-count classes x path x depth ---------------------------------------------------------------------
MS = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 192, 255, 256]
REP = {"half": 32, "zb1": 64, "zb2": 128, "zb4": 256}   # the count per class that also runs forced-fuse and the timed mode
P1, C1 = 4, 120

# id -> (P, C, M, depth, environment at phd_create, timed)
CLASS_CASES = {}
for _M in MS:
    for _env in ({}, {"PHD_CHAIN_MAX": "0"}):
        for _d in (False, True):
            CLASS_CASES["M%d-%s-%s-%s" % (_M, klass(_M), "depth" if _d else "nodepth", path_of(P1, _M, _env))] = (P1, C1, _M, _d, _env, False)
for _k, _M in REP.items():
    _env = {"PHD_CHAIN_MAX": "0", "PHD_FUSE_EP": "0" if zb_of(_M) == 1 else "1"}   # against the default of the class
    CLASS_CASES["M%d-%s-depth-%s-forced" % (_M, _k, path_of(P1, _M, _env))] = (P1, C1, _M, True, _env, False)
    CLASS_CASES["M%d-%s-depth-timed-%s" % (_M, _k, path_of(P1, _M, {}))] = (P1, C1, _M, True, {}, True)
# one particle at 256 measurements: the pinned measurement staging is exactly full (max(8 P + 8, 768) doubles)
CLASS_CASES["M256-zb4-nodepth-P1-staging-full-chain"] = (1, C1, 256, False, {}, False)
# the two-stream step (from 1024 particles) at four measurement blocks
for _d in (False, True):
    CLASS_CASES["M256-zb4-%s-P1024-separate-unfused-two-streams" % ("depth" if _d else "nodepth")] = (1024, 128, 256, _d, {}, False)


@pytest.mark.parametrize("case", list(CLASS_CASES))
def test_measurement_classes_against_the_oracle(monkeypatch, case):
    """stage parity on every particle with the frame's measurements (and an occluding map where the id says depth), three
    whole steps from the same state, then the path step"""
    P, C, M, depth, env, timed = CLASS_CASES[case]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    seed = 3000 + list(CLASS_CASES).index(case)
    f = frame(P, C, M, seed)
    nav, p = make(f)
    if timed:
        nav.set_frozen(True)
        nav.set_all_pairs(True)
    d0 = biting_map(p, oracle_state(f, p.max_quantity), f.z, seed, case) if depth else None
    # (1024 particles: the stages of every 16th — they run per particle; the whole steps below compare every one)
    stage_parity(nav, p, f, f.z, d0, stride=16 if P >= 1024 else 1)
    upload(nav, f)
    dlast = whole_steps(nav, p, f, seed, depth, timed, case)
    assert_path(nav, [(f.z, dlast)], launches(path_of(P, M, env), 2 if P >= 1024 else 1), case)
    nav.close()


# ---- 2. the measurement count changing between the steps of one handle -----------------------------------------------
SEQ = [30, 256, 0, 64, 65, 1, 129, 32, 33, 128]   # every class, both sides of every block boundary
SEQ_P = {"P8-chain": (8, 1), "P700-separate-one-stream": (700, 1), "P1024-separate-two-streams-pipelined": (1024, 2)}


def seq_plan(f, seed):
    """(measurements, u, depth map, whether the map changes before the step) per step: a map set before step 3, replaced
    before 4, kept through 5, cleared before 6"""
    rng = np.random.default_rng(seed)
    out, depth = [], None
    for s, m in enumerate(SEQ):
        z = perturbed(f.z[:m], rng)
        if s == 3:
            depth = occluder(seed)
        elif s == 4:
            depth = occluder(seed + 1)
        elif s == 6:
            depth = None
        out.append((z, float(rng.uniform(0.05, 0.95)), depth, s in (3, 4, 6)))
    return out


@pytest.mark.parametrize("drive", ["slam_update", "posted"])
@pytest.mark.parametrize("shape", list(SEQ_P))
def test_measurement_count_changes_between_steps(shape, drive):
    """one handle (max_measurements 256) through a sequence whose M walks every class: with SlamUpdate every step against
    the oracle; posted back to back (set_measurements + step_async, one sync at the end — from 1024 particles the two-stream
    pipelined step boundary) the final state and the last step's sources. Then the path: a HALF and a ZB4 step, timed."""
    P, streams = SEQ_P[shape]
    seed = 4100 + list(SEQ_P).index(shape)
    f = frame(P, 48, 256, seed)
    nav, p = make(f, max_measurements=256)
    st = oracle_state(f, p.max_quantity)
    plan = seq_plan(f, seed)
    for s, (z, u, depth, change) in enumerate(plan):
        with orc.depth_map(depth):
            best, src, res, _ = orc.slam_update(p, st, z, u=u, threads=THREADS)
        if change:
            nav.set_depth_map(depth)
        if drive == "slam_update":
            nav.SlamUpdate(None, z, u_resample=u)
            assert_step_matches(nav, st, best, src, res, p.max_quantity, "%s step %d (M %d)" % (shape, s, len(z)))
        else:
            nav.set_measurements(z)
            nav.step_async(u_resample=u)
    if drive == "posted":
        nav.sync()
        assert_step_matches(nav, st, best, src, res, p.max_quantity, "%s after %d posted steps" % (shape, len(plan)))
    want = {}
    for M in (32, 129):
        for k, n in launches(path_of(P, M, {}), streams).items():
            want[k] = want.get(k, 0) + n
    assert_path(nav, [(f.z[:32], None), (f.z[:129], None)], want, shape)
    nav.close()


# ---- 3. the sweep's component tiles and its compact birth sums -------------------------------------------------------
COMPONENT_COUNTS = [1, 2, 3, 4, 5, 7, 8, 9, 127, 128, 129, 255, 256, 257]
CM = [(C, M) for M in (32, 33, 65) for C in COMPONENT_COUNTS]


@pytest.mark.parametrize("C,M", CM, ids=["C%d-M%d-%s-chain" % (C, M, klass(M)) for C, M in CM])
def test_sweep_component_counts(C, M):
    """the tile ends of the sweep (128 components) and, under HALF, visits of two components (cc and cc + 4, clamped to
    the tile's last) on maps of 1 - 9 components"""
    f = frame(3, C, M, 4200 + C + 1000 * M)
    nav, p = make(f)
    stage_parity(nav, p, f, f.z)
    assert_path(nav, [(f.z, None)], launches("chain"), "C%d M%d" % (C, M))
    nav.close()


def birth_frame(P, C, M, u, late, seed):
    """C > 128 components. Pixel-range points: the ordinary components at ranges 0.3 - 0.85, `late` components (indices
    128 ...) at 1.38 - 1.42, u measurements at 1.93 - 1.99. A point at range r lies on the sphere of radius r around the
    camera, so the three groups are more than 0.5 apart: beyond the sweep's density gate (DensityDistanceThreshold).
    Measurements: M - u - late of the first tile's components (explained in the first tile), one of each late component
    (nothing of the first tile explains them: they close in the second), u of nothing (born)."""
    f = Frame(P, C, M, seed, weight_profile="steady")
    rng = np.random.default_rng(seed + 1)
    zc = np.stack([rng.uniform(-280, 280, C), rng.uniform(-200, 200, C), rng.uniform(0.3, 0.85, C)], axis=1)
    lc = 128 + np.arange(late)
    zc[lc, 2] = rng.uniform(1.38, 1.42, late)
    base = measure_to_map_identity(zc)
    f.mean = base[None] + rng.normal(size=(P, C, 3)) * 1e-3
    A = rng.uniform(-0.02, 0.02, size=(C, 3, 3))
    f.cov = np.broadcast_to(A @ np.transpose(A, (0, 2, 1)) + 1e-4 * np.eye(3), (P, C, 3, 3))
    f.w = np.broadcast_to(rng.uniform(0.3, 1.2, C), (P, C))
    nord = M - u - late
    zo = measure_perfect_identity(base[np.arange(nord) % 128]) + rng.normal(size=(nord, 3)) * [0.3, 0.3, 1e-3]
    zl = measure_perfect_identity(base[lc]) + rng.normal(size=(late, 3)) * [0.3, 0.3, 1e-3]
    zb = np.stack([rng.uniform(-300, 300, u), rng.uniform(-220, 220, u), rng.uniform(1.93, 1.99, u)], axis=1)
    kind = np.array([0] * nord + [1] * late + [2] * u)
    perm = rng.permutation(M)
    f.z = np.concatenate([zo, zl, zb])[perm]
    f.M = M
    return f, kind[perm]


def late_of(u):
    return 3 if u > 16 else min(3, 16 - u)


BIRTHS = [(u, M) for M in (24, 48, 100, 160) for u in (0, 15, 16, 17)]   # HALF, ZB1, ZB2, ZB4


@pytest.mark.parametrize("u,M", BIRTHS, ids=["u%d-late%d-M%d-%s-%s-chain" % (u, late_of(u), M, klass(M), "no-switch" if u > 16 else "compact")
                                             for u, M in BIRTHS])
def test_compact_birth_sums(u, M):
    """After the first tile u + late measurements are open: at most SW_UMAX = 16 and the sweep leaves the pair loop —
    the late ones close in the second tile through the compact sums (s_ulist / s_du), the u are born; 17 and it never
    switches. The oracle shows the frame is what it is built for: C + u predicted components, and no first-tile
    component within the gate of a late measurement."""
    late = late_of(u)
    C = 200
    f, kind = birth_frame(3, C, M, u, late, 4300 + u + M)
    nav, p = make(f)
    for i in range(f.P):
        pred = orc.predict(p, f.poses[i], f.z, f.map(i))
        assert len(pred[0]) == C + u, "particle %d: %d born, the frame is built for %d" % (i, len(pred[0]) - C, u)
        for k in np.nonzero(kind == 1)[0]:
            x = orc.measure_to_map(p, f.poses[i], f.z[k])
            assert np.min(np.linalg.norm(f.mean[i, :128] - x, axis=1)) > 0.5
            assert np.min(np.linalg.norm(f.mean[i, 128:] - x, axis=1)) < 0.05
    stage_parity(nav, p, f, f.z)
    assert_path(nav, [(f.z, None)], launches("chain"), "u%d M%d" % (u, M))
    nav.close()


def test_empty_map_all_measurements_born():
    """C = 0 and 256 measurements: every one is born, in one pass of the births loop (four blocks). The births' wide
    covariance gates every measurement with dozens of them: the corrected mixture outgrows the default emit_capacity
    (PHD_ERR_CAPACITY), so the handle gets room for every pair."""
    f = frame(3, 0, 256, 4400)
    nav, p = make(f, emit_capacity=256 * 257)
    want = stage_parity(nav, p, f, f.z)
    assert all(len(w[0][0]) == 256 for w in want)
    assert_path(nav, [(f.z, None)], launches("chain"), "C0-M256-zb4")
    nav.close()


# ---- 4. the bound of the quasi set log-likelihood's landmark set -----------------------------------------------------
@pytest.mark.parametrize("maxq,jcap", [(600, 640), (1100, 1024)])
def test_quasi_landmark_bound_is_the_landmark_scratch(maxq, jcap):
    """include/phdhip.h: nlandmarks <= min(1024, max_quantity rounded up to a multiple of 64) — Jcap landmarks are taken
    (their values against the oracle: tests/test_gpu_parity.py, J = Jcap), one more is PHD_ERR_BAD_ARGUMENT"""
    from monorfs_amd import navigator
    f = frame(4, jcap + 1, 8, 4500 + maxq)
    nav, p = make(f, maxq=maxq)
    lm, z = f.mean[0], f.z
    got = nav.QuasiSetLogLikelihood(z, lm[:jcap], f.poses)
    want = [orc.quasi_set_log_likelihood(p, f.poses[i], lm[:jcap], z) for i in range(f.P)]
    assert np.allclose(got, want, rtol=1e-9, atol=1e-9)
    for call in (lambda: nav.QuasiSetLogLikelihood(z, lm, f.poses), lambda: nav.QuasiSetLogLikelihoodGradient(z, lm, f.poses)):
        with pytest.raises(navigator.PHDError) as e:
            call()
        assert e.value.status == PHD_ERR_BAD_ARGUMENT
    nav.close()


# ---- 5. the landmark count J = (int) ExpectedSize of WeightAlpha ------------------------------------------------------
def alpha_frame(n_in, w_in, n_det, wo, seed, P=2):
    """n_in in-view components on a pixel grid (ranges 0.6 - 1.6) of prior weight w_in, the first n_det of them measured;
    len(wo) out-of-view ones beyond the film's right edge (pixel x 450 - 1300: detection probability 0, the correction
    leaves their weights wo as they are) — they tune ExpectedSize. Small covariances, grid spacing far beyond the merge
    distance."""
    n_out = len(wo)
    gx = max(1, int(np.ceil(np.sqrt(n_in * 4 / 3))))
    gy = max(1, int(np.ceil(n_in / gx)))
    xs, ys = np.meshgrid(np.linspace(-280, 280, gx), np.linspace(-200, 200, gy))
    zin = np.stack([xs.ravel()[:n_in], ys.ravel()[:n_in], 0.6 + (np.arange(n_in) % 5) * 0.25], axis=1)
    ox, oy, orr = np.meshgrid(np.linspace(450, 1300, 10), np.linspace(-240, 240, 20), [0.6, 1.0, 1.4], indexing="ij")
    zout = np.stack([ox.ravel(), oy.ravel(), orr.ravel()], axis=1)[:n_out]
    C = n_in + n_out
    f = Frame(P, C, max(n_det, 1), seed, weight_profile="steady")
    base = measure_to_map_identity(np.concatenate([zin, zout]))
    rng = np.random.default_rng(seed)
    f.mean = base[None] + rng.normal(size=(P, C, 3)) * 1e-4
    f.cov = np.broadcast_to(2.5e-5 * np.eye(3), (P, C, 3, 3))
    f.w = np.broadcast_to(np.concatenate([np.full(n_in, w_in), np.asarray(wo, float)]), (P, C))
    f.M = n_det
    f.z = measure_perfect_identity(base[:n_det]) + rng.normal(size=(n_det, 3)) * [0.3, 0.3, 1e-3]
    return f


def oracle_pruned(p, f, i):
    pred = orc.predict(p, f.poses[i], f.z, f.map(i))
    return pred, orc.prune(p, orc.correct(p, f.poses[i], f.z, pred))


def seq_sum(w):
    """the reference's ExpectedSize: the weights added one by one in map order"""
    s = 0.0
    for x in w:
        s += float(x)
    return s


def tree_sum(w):
    """k_alpha_assoc's ExpectedSize before its re-add: 256 thread partials in map order (c = t, t + 256, ...), then a tree"""
    red = np.array([seq_sum(w[t::256]) for t in range(256)])
    s = 128
    while s:
        red[:s] = red[:s] + red[s:2 * s]
        s >>= 1
    return float(red[0])


def tuned(p, f, n_out, total):
    """f with its out-of-view weights scaled so that particle 0's pruned map sums to `total`; they stay lighter than every
    in-view component after the correction, so the J-th pick is in view"""
    _, pr = oracle_pruned(p, f, 0)
    w = np.array(f.w[0])
    wo = w[-n_out:]
    inside = seq_sum(pr[0]) - seq_sum(wo)
    w[-n_out:] = wo * ((total - inside) / seq_sum(wo))
    if w[-n_out:].min() < p.min_weight:
        return None
    f.w = np.broadcast_to(w, f.w.shape)
    return f


def jth_in_view(p, f, i):
    """the last landmark of the oracle's map estimate of particle i lies inside the film"""
    lm, _ = orc.best_map_estimate(oracle_pruned(p, f, i)[1])
    return abs(orc.measure_perfect(p, f.poses[i], lm[-1])[0]) < 320


def setll_and_j(p, f, i):
    pred, pr = oracle_pruned(p, f, i)
    return orc.weight_alpha(p, f.poses[i], f.z, pred, pr)[1], len(orc.best_map_estimate(pr)[0])


# id -> (J, in-view components, their prior weight, measured, out-of-view components). PD 0.2: a few hundred undetected
# landmarks keep alpha far above the smallest double.
ALPHA_CASES = {
    "J0-chain": (0, 1, 0.5, 0, 10),
    "J13-beyond-7-components-chain": (13, 3, 5.375, 0, 4),     # in-view weights 4.3 after the correction: each picked 5 times
    "J256-lds-chain": (256, 262, 1.1, 8, 40),
    "J257-hbm-slab-chain": (257, 262, 1.1, 8, 40),
}


@pytest.mark.parametrize("case", list(ALPHA_CASES))
def test_alpha_landmark_count(case):
    """the pruned maps put J where the id says (the oracle's BestMapEstimate), the J-th pick is in view, and the set
    log-likelihood with J - 1 and J + 1 (the out-of-view weights moved by one in total, where they stay above MinWeight) is
    far from the one with J — the witness of the J-th pick. (Alpha does not show it: for an undetected landmark the
    misdetection factor of the set likelihood cancels against the density ratio of WeightAlpha, to 1e-13 here.) Then the
    stages, alpha and the set log-likelihood against the oracle."""
    J, n_in, w_in, n_det, n_out = ALPHA_CASES[case]
    seed = 4600 + list(ALPHA_CASES).index(case)
    p = prm3d_defaults(max_particles=2, max_components=600, max_measurements=max(n_det, 1))
    p.pd = 0.2
    a = {}
    for dj in (-1, 1, 0):
        f = tuned(p, alpha_frame(n_in, w_in, n_det, np.full(n_out, 0.01), seed), n_out, J + dj + 0.5)
        if f is None:
            assert dj != 0
            continue
        for i in range(f.P):
            a[dj, i], j = setll_and_j(p, f, i)
            assert j == J + dj, "particle %d: the map estimate has %d landmarks, the case is built for %d" % (i, j, J + dj)
    for i in range(f.P):
        assert J == 0 or jth_in_view(p, f, i), "particle %d: the J-th pick is out of view" % i
        assert (-1, i) in a or (1, i) in a
        for dj in (-1, 1):
            if (dj, i) in a:
                assert abs(a[dj, i] - a[0, i]) > 0.1, "the set log-likelihood does not change with the J-th pick"
    nav, p = make(f, pd=0.2)
    stage_parity(nav, p, f, f.z)
    assert_path(nav, [(f.z, None)], launches("chain"), case)
    nav.close()


def test_alpha_landmark_count_next_to_an_integer():
    """ExpectedSize a few ulp from an integer, the map-order sum on one side and k_alpha_assoc's tree sum on the other
    (searched on the host): only the re-add in map order (phd_alpha.h) gives the reference's J"""
    n_in, w_in, n_out, J = 44, 1.1, 60, 40
    p = prm3d_defaults(max_particles=1, max_components=600, max_measurements=1)
    p.pd = 0.2
    rng = np.random.default_rng(4700)
    found = None
    for _ in range(300):
        f = tuned(p, alpha_frame(n_in, w_in, 0, rng.uniform(0.01, 0.04, n_out), 4700, P=1), n_out, float(J))
        for _ in range(4):
            pw = oracle_pruned(p, f, 0)[1][0]
            s, t = seq_sum(pw), tree_sum(pw)
            if (s < J) != (t < J):
                found = f
                break
            if s == t:
                break
            w = np.array(f.w[0])
            w[-1] += J - 0.5 * (s + t)
            f.w = w[None]
        if found is not None:
            break
    assert found is not None, "no weights put the two sums on both sides of %d" % J
    f = found
    s = seq_sum(oracle_pruned(p, f, 0)[1][0])
    assert abs(s - J) <= 1e-9 * J   # (where the device re-adds)
    _, j = setll_and_j(p, f, 0)
    assert j == int(s) and j in (J - 1, J)
    nav, p = make(f, pd=0.2, max_measurements=1)
    stage_parity(nav, p, f, f.z)
    assert_path(nav, [(f.z, None)], launches("chain"), "J next to an integer")
    nav.close()


def test_alpha_landmark_count_beyond_the_scratch():
    """600 out-of-view components of weight 1.1, no measurements: ExpectedSize 660 > Jcap = 640 at max_quantity 600 — the
    step is PHD_ERR_CAPACITY and leaves weights and maps bit for bit; at max_quantity 1100 (Jcap 1024, the HBM slab) the
    same step matches the oracle"""
    from monorfs_amd import navigator
    f = alpha_frame(0, 1.0, 0, np.full(600, 1.1), 4800)
    f.weights = np.array([0.3, 0.7])   # (the two maps weigh the same: distinct particle weights keep BestParticle well-posed)
    nav, p = make(f, max_measurements=1)
    before = nav.download_state(600)
    with pytest.raises(navigator.PHDError) as e:
        nav.SlamUpdate(None, f.z, u_resample=0.5)
    assert e.value.status == PHD_ERR_CAPACITY and "landmark scratch" in str(e.value)
    after = nav.download_state(600)
    for x, y in zip(before, after):
        assert np.array_equal(x, y)
    nav.close()
    nav, p = make(f, maxq=1100, max_measurements=1)
    st = oracle_state(f, p.max_quantity)
    assert len(orc.best_map_estimate(st.map(0))[0]) == 660
    best, src, res, _ = orc.slam_update(p, st, f.z, u=0.5, threads=THREADS)
    nav.SlamUpdate(None, f.z, u_resample=0.5)
    assert_step_matches(nav, st, best, src, res, p.max_quantity, "J 660 at Jcap 1024")
    assert_path(nav, [(f.z, None)], launches("chain"), "J 660")
    nav.close()
