"""PruneModel (PHDNavigator.cs:913-948) once more, in plain numpy, and the maps that take its merge half down every path
the device's prune_merge_body (monorfs_amd/csrc/phd_prune.h) has for it. No GPU and no oracle in here.

ref_prune is the second reading of the oracle's `prune` (tests/test_oracle_prune_paths.py holds the two against each
other, to the bit) and says of every case what the case is FOR: the rows in the cut, how many later rows each row is close
to, who absorbed whom, how often a close row was already gone. Each family below carries conditions on those figures —
asserted from the reference alone, never from the device —, so that a case that no longer reaches its path fails instead
of passing for nothing. The paths (phases B and C of the kernel body):
  * the lane-per-row walk of the candidates with its queue of eight pending rows (up to PRUNE_HEAVY = 32 candidates),
  * the wave-per-row walk of a row with more candidates than that,
  * the full scan of a row whose covariance is not positive definite,
  * the re-test of a row with more than PRUNE_NBR = 7 close rows by the resolving wave,
  * the slab reads of the means from row 1024 on, the absorbed flags from row 2048 on.

Two conditions hold for every case, because the device inverts P_i in float64 by another route than either reading: no
tested pair lies closer to the threshold than 1e-6 (relative, in the squared Mahalanobis distance), and no positive
definite covariance has a condition number above 1e4. A builder draws again, from the next seed, until both hold."""
import functools

import numpy as np

MERGE_THRESHOLD = 0.3      # Config.cs:84
MIN_WEIGHT = 1e-3          # Config.cs:253
PRUNE_NBR = 7              # phd_prune.h: close rows a row keeps in its list
PRUNE_HEAVY = 32           # phd_prune.h: candidates up to which one lane walks a row
MARGIN = 1e-6
MAX_CONDITION = 1e4
L = np.longdouble


class Info:
    """what ref_prune saw: all row numbers are ranks (positions in the sorted, cut list)"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def absorbed(self):
        return np.flatnonzero(self.owner >= 0)


def ref_prune(w, mean, cov, min_weight, max_quantity, merge_threshold):
    """PruneModel as PHDNavigator.cs:913-948 reads: a stable sort by falling weight (List.Sort's comparator made stable by
    the canonical index), the cut at min(MaxQuantity, first weight < MinWeight), then every still-present row i absorbs
    every later still-present row k with (m_i - m_k)^T P_i^-1 (m_i - m_k) < T^2 — P_i alone: the test is not symmetric —
    and leaves Gaussian.Merge of itself and its members, in rank order.

    The closeness decisions are taken in np.longdouble with the 3 x 3 inverse by adjugate / determinant; the moments of
    Gaussian.Merge in float64 in the reference's order of summation (Gaussian.cs:329-346, its W < 1e-15 branch too).
    Returns (weights, means, covariances, Info)."""
    w = np.asarray(w, np.float64)
    mean = np.asarray(mean, np.float64).reshape(-1, 3)
    cov = np.asarray(cov, np.float64).reshape(-1, 3, 3)
    order = np.argsort(-w, kind="stable")
    limit = min(int(max_quantity), len(w))
    below = np.flatnonzero(w[order][:limit] < min_weight)
    cut = int(below[0]) if len(below) else limit
    order = order[:cut]
    sw, sm, sP = w[order], mean[order], cov[order]

    m, P = sm.astype(L), sP.astype(L)
    a, b, c, d, e, f, g, h, i_ = (P[:, r, s] for r in range(3) for s in range(3))
    adj = np.empty((cut, 3, 3), L)
    adj[:, 0, 0], adj[:, 0, 1], adj[:, 0, 2] = e * i_ - f * h, c * h - b * i_, b * f - c * e
    adj[:, 1, 0], adj[:, 1, 1], adj[:, 1, 2] = f * g - d * i_, a * i_ - c * g, c * d - a * f
    adj[:, 2, 0], adj[:, 2, 1], adj[:, 2, 2] = d * h - e * g, b * g - a * h, a * e - b * d
    det = a * adj[:, 0, 0] + b * adj[:, 1, 0] + c * adj[:, 2, 0]
    T2 = L(merge_threshold) * L(merge_threshold)
    eig = np.linalg.eigvalsh(sP) if cut else np.zeros((0, 3))
    pd = eig[:, 0] > 0 if cut else np.zeros(0, bool)
    bound = float(merge_threshold) ** 2 * np.trace(sP, axis1=1, axis2=2) if cut else np.zeros(0)

    close, margin = [], np.inf
    nclose, inball = np.zeros(cut, int), np.zeros(cut, int)
    for i in range(cut):
        inv = adj[i] / det[i]
        D = m[i] - m
        q = (D[:, 0] * (inv[0, 0] * D[:, 0] + inv[0, 1] * D[:, 1] + inv[0, 2] * D[:, 2]) +
             D[:, 1] * (inv[1, 0] * D[:, 0] + inv[1, 1] * D[:, 1] + inv[1, 2] * D[:, 2]) +
             D[:, 2] * (inv[2, 0] * D[:, 0] + inv[2, 1] * D[:, 1] + inv[2, 2] * D[:, 2]))
        later = q[i + 1:]
        if len(later):
            margin = min(margin, float(np.min(np.abs(later - T2)) / T2))
        close.append(i + 1 + np.flatnonzero(later < T2))
        nclose[i] = len(close[i])
        # rows (earlier and later ones) inside the Euclidean bound |d|^2 <= T^2 trace(P_i): the least a grid can hand row i
        inball[i] = (np.count_nonzero((D * D).sum(axis=1).astype(np.float64) <= bound[i]) - 1) if pd[i] else -1

    owner, skipped = np.full(cut, -1), 0
    ow, om, oc = [], [], []
    for i in range(cut):
        if owner[i] >= 0:
            continue
        members = [i]
        for k in close[i]:
            if owner[k] >= 0:
                skipped += 1
            else:
                owner[k] = i
                members.append(int(k))
        W, M, Cv = 0.0, np.zeros(3), np.zeros((3, 3))
        for k in members:
            W = W + sw[k]
            M = M + sw[k] * sm[k]
            Cv = Cv + sw[k] * (sP[k] + np.outer(sm[k], sm[k]))
        if W < 1e-15:     # Gaussian.cs:339-341, Util.InfiniteCovariance
            ow.append(0.0), om.append(sm[i].copy()), oc.append(np.diag([1e12, 1e12, 1e12]))
        else:
            M = M / W
            ow.append(W), om.append(M), oc.append(Cv / W - np.outer(M, M))
    n = len(ow)
    info = Info(cut=cut, order=order, nclose=nclose, close=close, owner=owner, skipped=skipped, margin=margin, inball=inball,
                positive_definite=pd, condition=np.where(pd, eig[:, 2] / np.where(pd, eig[:, 0], 1.0), 0.0) if cut else np.zeros(0),
                radius=np.sqrt(np.where(pd, bound, 0.0)), infinite=int(np.count_nonzero(np.array(ow) == 0.0)) if n else 0)
    return np.array(ow).reshape(n), np.array(om).reshape(n, 3), np.array(oc).reshape(n, 3, 3), info


# ---- the cases ----------------------------------------------------------------------------------------------------------------
class Case:
    """a map for PruneModel: (w, mean, cov, max_quantity) — `tuple(case)` —, the MinWeight it is pruned at and the capacity a
    handle needs for it (a multiple of 64 that holds the map and MaxQuantity)"""

    def __init__(self, w, mean, cov, max_quantity, min_weight=MIN_WEIGHT):
        self.w, self.mean = np.asarray(w, np.float64), np.asarray(mean, np.float64)
        c = np.asarray(cov, np.float64)
        self.cov = 0.5 * (c + c.transpose(0, 2, 1))
        self.max_quantity, self.min_weight = int(max_quantity), float(min_weight)
        self.capacity = ((max(len(self.w), self.max_quantity) + 63) // 64) * 64

    def __iter__(self):
        return iter((self.w, self.mean, self.cov, self.max_quantity))

    def mix(self):
        return self.w, self.mean, self.cov


def rotations(rng, n):
    q, r = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    return q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]


def rotated_covs(rng, n, lo, hi):
    """n covariances R diag(e) R^T: R a random rotation, the eigenvalues log-uniform in [lo, hi]"""
    R = rotations(rng, n)
    e = np.exp(rng.uniform(np.log(lo), np.log(hi), (n, 3)))
    return np.einsum("nij,nj,nkj->nik", R, e, R)


def iso(n, var=0.01):
    return np.broadcast_to(np.eye(3) * var, (n, 3, 3)).copy()


def weights(rng, n, lo=0.01, hi=1.0):
    return rng.uniform(lo, hi, n)


def merge_distance(var):
    return MERGE_THRESHOLD * np.sqrt(var)


def chain(seed, shuffled):
    """40 rows on a line, 2/3 of the merge distance apart, the weights falling along it: every row is close to its next one
    only, so row 1 goes to row 0 and, absorbed, must leave row 2 alone (an absorbed row absorbs nothing). Shuffled, the
    ranks jump about the line and a row finds close rows that an earlier leader already took (phase C's `km` test)."""
    rng = np.random.default_rng(seed)
    n, step = 40, merge_distance(0.01) * 2 / 3
    direction = rotations(rng, 1)[0][:, 0]
    mean = np.array([0.3, -0.2, 0.9]) + np.arange(n)[:, None] * step * direction
    w = np.sort(weights(rng, n))[::-1].copy()
    if shuffled:
        w = w[rng.permutation(n)]
    return Case(w, mean, iso(n), 600)


def check_chain(case, info, shuffled):
    assert info.cut == 40
    # an absorbed row with a close later row that it must not take: that row leads, or went to somebody else
    assert any(info.owner[i] >= 0 and any(info.owner[k] != i for k in info.close[i]) for i in range(info.cut))
    assert all(info.owner[info.owner[k]] < 0 for k in info.absorbed)
    if shuffled:
        assert info.skipped > 0, info.skipped
    else:
        assert len(info.absorbed) == 20 and info.skipped == 0


def small_crowd(seed):
    """32 rows in all, two clusters of 20 and 12: no row has more than PRUNE_HEAVY candidates whatever the grid makes of
    them, so every row is walked by one lane; the heaviest row of the larger cluster is close to 8 or more later rows — its
    queue of eight drains in the middle of the walk, and the resolving wave re-tests it (more than PRUNE_NBR)."""
    rng = np.random.default_rng(seed)
    centres = np.array([[0.2, 0.1, 0.8], [0.9, -0.4, 1.3]])
    mean = np.concatenate([centres[0] + rng.normal(size=(20, 3)) * 0.012, centres[1] + rng.normal(size=(12, 3)) * 0.02])
    return Case(weights(rng, 32), mean, rotated_covs(rng, 32, 0.004, 0.02), 600)


def check_small_crowd(case, info):
    assert info.cut <= PRUNE_HEAVY
    leaders = np.flatnonzero(info.owner < 0)
    assert any(PRUNE_NBR < info.nclose[i] <= 32 for i in leaders), info.nclose[leaders]
    assert any(0 < info.nclose[i] <= PRUNE_NBR for i in leaders), info.nclose[leaders]


def crowd(seed):
    """6 clusters of 50 rows with random rotated covariances: the leaders have 33 and more rows inside their Euclidean
    bound, so their candidates are spread over a wave whatever cells the grid cuts, and more than PRUNE_NBR close rows"""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-1.5, 1.5, (6, 3))
    mean = (centres[:, None, :] + rng.normal(size=(6, 50, 3)) * 0.02).reshape(-1, 3)
    return Case(weights(rng, 300), mean, rotated_covs(rng, 300, 0.003, 0.02), 600)


def check_crowd(case, info):
    leaders = np.flatnonzero(info.owner < 0)
    assert any(info.inball[i] > PRUNE_HEAVY and info.nclose[i] > PRUNE_NBR for i in leaders)
    assert len(info.absorbed) > 100


def one_wide(seed):
    """600 narrow rows and one whose covariance is 1e4 times wider: the wide row's radius sets the cell size for all, and
    dozens of rows lie inside its bound; the narrow rows, all in a few cells now, still merge with true neighbours only"""
    rng = np.random.default_rng(seed)
    n = 600
    mean = rng.uniform(-0.5, 0.5, (n + 1, 3))
    mean[450:600] = mean[300:450] + rng.normal(size=(150, 3)) * 1.5e-3     # 150 narrow rows with a true neighbour each
    cov = np.concatenate([rotated_covs(rng, n, 7e-5, 1.4e-4), rotated_covs(rng, 1, 0.7, 1.4)])
    w = np.concatenate([weights(rng, n), [0.5]])
    return Case(w, mean, cov, 640)


def check_one_wide(case, info):
    wide = int(np.argmax(info.radius))
    assert info.radius[wide] > 50 * np.sort(info.radius)[-2]
    assert info.inball[wide] > PRUNE_HEAVY
    narrow = np.flatnonzero(np.arange(info.cut) != wide)
    merged = [i for i in narrow if info.owner[i] < 0 and info.nclose[i] > 0]
    assert len(merged) >= 5 and info.nclose[narrow].max() < 20, (len(merged), info.nclose[narrow].max())
    assert np.count_nonzero(info.owner < 0) > 300


def same_mean(seed):
    """300 rows with one and the same mean (an extent of 0: the cell size comes from the radius alone, every row is a
    candidate of every row): the heaviest takes the other 299"""
    rng = np.random.default_rng(seed)
    mean = np.broadcast_to(np.array([0.4, -0.3, 1.1]), (300, 3)).copy()
    return Case(weights(rng, 300), mean, rotated_covs(rng, 300, 0.003, 0.02), 600)


def check_same_mean(case, info):
    assert np.count_nonzero(info.owner < 0) == 1 and len(info.absorbed) == 299 and info.nclose[0] == 299


def aniso_threshold(seed):
    """one leader with the covariance R diag(1, 1e-3, 1e-3) R^T and light, narrow partners: along its major axis at
    0.3 (1 -+ 1e-3) on both sides — just inside and just outside the merge distance, where the Euclidean bound
    T^2 trace(P) is at its tightest (T^2 1.002 against |d|^2 = T^2 (1 -+ 1e-3)^2) —, across it at 0.9 and 1.1 of the minor
    merge distance. Exactly the inside ones are absorbed."""
    rng = np.random.default_rng(seed)
    R = rotations(rng, 1)[0]
    lead = R @ np.diag([1.0, 1e-3, 1e-3]) @ R.T
    centre = np.array([0.5, 0.2, 1.0])
    minor = MERGE_THRESHOLD * np.sqrt(1e-3)
    offs = [s * MERGE_THRESHOLD * (1 + t * 1e-3) * R[:, 0] for s in (1, -1) for t in (-1, 1)]
    offs += [s * f * minor * R[:, ax] for ax in (1, 2) for s in (1, -1) for f in (0.9, 1.1)]
    inside = [t < 0 for s in (1, -1) for t in (-1, 1)] + [f < 1 for ax in (1, 2) for s in (1, -1) for f in (0.9, 1.1)]
    mean = np.concatenate([[centre], centre + np.array(offs)])
    n = len(mean)
    cov = np.concatenate([[lead], iso(n - 1, 1e-9)])
    w = np.concatenate([[1.0], np.sort(weights(rng, n - 1, 0.01, 0.5))[::-1]])
    case = Case(w, mean, cov, 600)
    case.inside = np.array(inside)
    return case


def check_aniso_threshold(case, info):
    assert info.cut == 13 and info.order[0] == 0
    assert np.array_equal(info.owner[1:] == 0, case.inside[info.order[1:] - 1])
    assert np.count_nonzero(info.owner == 0) == 6 and not np.any(info.owner > 0)
    assert info.margin < 3e-3      # (the pairs at 0.3 (1 -+ 1e-3): 2e-3 from the threshold)


def far_extent(seed):
    """8 clusters of 20 rows, 5 km apart, covariances of 5e-5 to 2e-4 (merge distances of 2 to 4 mm): the float32 copies
    the pair search walks are coarser (2^-24 x extent = 3e-4 m) than a tenth of the merge distance — the margin `ferr` is
    what keeps a close pair among the candidates"""
    rng = np.random.default_rng(seed)
    corners = np.array([[x, y, z] for x in (0.0, 5000.0) for y in (0.0, 5000.0) for z in (0.0, 5000.0)]) + rng.uniform(-1, 1, (8, 3))
    mean = (corners[:, None, :] + rng.normal(size=(8, 20, 3)) * 2.5e-3).reshape(-1, 3)
    return Case(weights(rng, 160), mean, rotated_covs(rng, 160, 5e-5, 2e-4), 600)


def check_far_extent(case, info):
    extent = np.ptp(case.mean, axis=0).max()
    assert 2.0 ** -24 * extent > 1e-4
    assert len(info.absorbed) > 50, len(info.absorbed)
    assert info.radius.max() < 0.01


def indefinite(seed):
    """200 rows; the three heaviest have an invertible INDEFINITE covariance (eigenvalues 0.01, 0.01, -0.01, rotated). The
    boundary does not ask for definiteness and the oracle is defined there: d^T P^-1 d is negative inside a double cone,
    so such a row is close to rows at any distance — no Euclidean bound, every later row is tested (the full scan)"""
    rng = np.random.default_rng(seed)
    n = 200
    mean = rng.uniform(-0.4, 0.4, (n, 3))
    cov = rotated_covs(rng, n, 0.003, 0.02)
    R = rotations(rng, 3)
    cov[:3] = np.einsum("nij,j,nkj->nik", R, np.array([0.01, 0.01, -0.01]), R)
    w = weights(rng, n, 0.01, 0.8)
    w[:3] = [0.99, 0.95, 0.9]
    return Case(w, mean, cov, 600)


def check_indefinite(case, info):
    assert list(info.order[:3]) == [0, 1, 2] and not info.positive_definite[:3].any() and info.positive_definite[3:].all()
    assert info.owner[0] < 0 and info.nclose[0] > PRUNE_NBR
    assert np.count_nonzero(info.owner < 0) > 50


def tiny_total(seed):
    """MinWeight 1e-20: a cluster of five rows whose weights sum to 5e-16 and a lone row of 1e-17 — Gaussian.Merge's total
    below 1e-15 (Gaussian.cs:339-341: weight 0, the first mean, InfiniteCovariance) — among 30 ordinary rows"""
    rng = np.random.default_rng(seed)
    mean = rng.uniform(-1, 1, (36, 3))
    mean[30:35] = np.array([0.1, 0.2, 1.5]) + rng.normal(size=(5, 3)) * 0.004
    mean[35] = [3.0, 3.0, 3.0]
    w = np.concatenate([weights(rng, 30), rng.uniform(0.8e-16, 1.2e-16, 5), [1e-17]])
    return Case(w, mean, iso(36), 600, min_weight=1e-20)


def check_tiny_total(case, info):
    assert info.cut == 36 and info.infinite == 2
    assert np.count_nonzero(info.owner == 30) == 4


def uniform_box(seed, n, side, max_quantity):
    rng = np.random.default_rng(seed)
    return Case(weights(rng, n), rng.uniform(0, side, (n, 3)), rotated_covs(rng, n, 0.006, 0.014), max_quantity)


def past_1024(seed):
    """1300 rows uniform in a 1.2 m box, MaxQuantity 1344: rows from 1024 on are not in a thread's registers — grid, pair
    search and merge read their means back from the slab"""
    return uniform_box(seed, 1300, 1.2, 1344)


def check_past_1024(case, info):
    assert info.cut == 1300 and np.count_nonzero(info.absorbed >= 1024) >= 10


def past_2048(seed):
    """2300 rows uniform in a 1.5 m box, MaxQuantity 2304: absorbed rows on both sides of the 32 x 64 rows that one 32-bit
    word per lane holds flags for — a row k below rows - 2048 (whose flag must not take row k + 2048 with it) and a row
    from 2048 on (whose flag must not land on row k - 2048)"""
    return uniform_box(seed, 2300, 1.5, 2304)


def check_past_2048(case, info):
    assert info.cut == 2300
    assert np.count_nonzero(info.absorbed < info.cut - 2048) >= 1 and np.count_nonzero(info.absorbed >= 2048) >= 1
    # ... and the wrap would show: the twin row 2048 away of some absorbed row is not absorbed itself
    a = info.absorbed
    twins = np.concatenate([a[a + 2048 < info.cut] + 2048, a[a >= 2048] - 2048])
    assert np.any(info.owner[twins] < 0)


def top_max_quantity():
    """the largest multiple of 64 that phd_create takes as MaxQuantity with 8 measurements: the bound is the LDS of one
    workgroup, checked before a device is looked for, so the library answers without one"""
    import ctypes
    from monorfs_amd import _lib
    from monorfs_amd.abi import prm3d_defaults
    lib = _lib.load()
    for rows in range(3328, 0, -64):
        p = prm3d_defaults(1, rows, 8)
        p.max_quantity = rows
        h = lib.phd_create(ctypes.byref(p), 0)
        if h:
            lib.phd_destroy(h)
            return rows
        if b"max_quantity too large" not in lib.phd_create_error():
            return rows
    raise AssertionError("phd_create takes no MaxQuantity at all")


def near_the_top(seed):
    """as many rows as phd_create admits (the largest multiple of 64, stepping down from 3328), uniform in a box of the
    same density: absorbed rows below rows - 2048, from 2048 on and from 3072 on"""
    rows = top_max_quantity()
    return uniform_box(seed, rows, 1.5 * (rows / 2300.0) ** (1.0 / 3), rows)


def check_near_the_top(case, info):
    assert info.cut == len(case.w) == case.max_quantity >= 3072
    a = info.absorbed
    assert np.count_nonzero(a < info.cut - 2048) >= 1 and np.count_nonzero(a >= 2048) >= 1 and np.count_nonzero(a >= 3072) >= 1
    twins = np.concatenate([a[a + 2048 < info.cut] + 2048, a[a >= 2048] - 2048])
    assert np.any(info.owner[twins] < 0)


def sweep(seed, sparse):
    """200 to 700 rows with random rotated covariances. Dense: a box a few dozen radii wide — the cell size comes from the
    largest radius (2.02 r_max > extent / 60). Sparse: pairs and triples scattered over a box hundreds of radii wide — the
    cell size is extent / 60 and most cells are empty."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(200, 701))
    cov = rotated_covs(rng, n, 0.002, 0.02)
    if sparse:
        k = n // 3
        sites = rng.uniform(-6.0, 6.0, (k, 3))
        mean = sites[rng.integers(0, k, n)] + rng.normal(size=(n, 3)) * 0.015
    else:
        mean = rng.uniform(0, 0.09 * n ** (1.0 / 3), (n, 3))
    return Case(weights(rng, n), mean, cov, 704)


def check_sweep(case, info, sparse):
    assert 200 <= info.cut <= 700 and len(info.absorbed) >= 5
    extent = np.ptp(case.mean, axis=0).max()
    from_radius = 2.02 * info.radius.max() > extent / 60.0
    assert from_radius != sparse, (info.radius.max(), extent)


FAMILIES = {   # id -> (builder, check)
    "chain": (lambda s: chain(s, False), lambda c, i: check_chain(c, i, False)),
    "chain-shuffled": (lambda s: chain(s, True), lambda c, i: check_chain(c, i, True)),
    "small_crowd": (small_crowd, check_small_crowd),
    "crowd": (crowd, check_crowd),
    "one_wide": (one_wide, check_one_wide),
    "same_mean": (same_mean, check_same_mean),
    "aniso_threshold": (aniso_threshold, check_aniso_threshold),
    "far_extent": (far_extent, check_far_extent),
    "indefinite": (indefinite, check_indefinite),
    "tiny_total": (tiny_total, check_tiny_total),
    "past_1024": (past_1024, check_past_1024),
    "past_2048": (past_2048, check_past_2048),
    "near_the_top": (near_the_top, check_near_the_top),
}
for _seed in range(8):
    FAMILIES["sweep-dense-%d" % _seed] = ((lambda s, b=_seed: sweep(1000 * b + s, False)), lambda c, i: check_sweep(c, i, False))
    FAMILIES["sweep-sparse-%d" % _seed] = ((lambda s, b=_seed: sweep(1000 * b + s, True)), lambda c, i: check_sweep(c, i, True))

IDS = list(FAMILIES)


def sound(info):
    """the two conditions every case meets"""
    return info.margin >= MARGIN and info.condition.max() <= MAX_CONDITION


@functools.lru_cache(maxsize=None)
def built(name):
    """(case, reference result) of a family: drawn again from the next seed until the case is `sound`; the family's own
    conditions are then ASSERTED — a family that cannot meet them is a broken test, not a reason to draw again. Computed
    once per process and shared; nobody writes to it."""
    builder, check = FAMILIES[name]
    for seed in range(20):
        case = builder(seed)
        ref = ref_prune(case.w, case.mean, case.cov, case.min_weight, case.max_quantity, MERGE_THRESHOLD)
        if sound(ref[3]):
            break
    else:
        raise AssertionError("%s: no seed keeps every pair %g away from the threshold" % (name, MARGIN))
    info = ref[3]
    assert info.margin >= MARGIN and info.condition.max() <= MAX_CONDITION
    check(case, info)
    for x in (case.w, case.mean, case.cov) + ref[:3]:
        x.setflags(write=False)
    return case, ref


# ---- phase A: which ordering the weights of a map take -------------------------------------------------------------------------
# The branches of prune_order (phd_prune.h), decided from the weights alone: the bins are weight_bin_of_bits (phd_device.h)
# restated, NS and capN are PruneLds's, 512 is the most entries the ranked ordering ranks inside one bin.
def weight_bins(w, min_weight):
    """exponent and five mantissa bits of a positive double, counted from MinWeight's own bin up, clamped to 1024 bins"""
    k = (np.asarray(w, np.float64).view(np.uint64) << np.uint64(1)) >> np.uint64(48)
    base = (np.array([min_weight], np.float64).view(np.uint64) << np.uint64(1)) >> np.uint64(48)
    return np.clip(k.astype(np.int64) - int(base[0]), 0, 1023)


def order_branch(w, max_quantity, min_weight=MIN_WEIGHT):
    """(branch, ne, sort width): 'registers', 'ranked', 'ranked-rounds', 'one-pass', 'passes' or 'passes-refill'"""
    w = np.asarray(w, np.float64)
    w = w[w >= min_weight]                  # what the correction step emits
    ne, cut = len(w), min(int(max_quantity), len(w))
    NS = 512
    while NS < 2 * int(max_quantity):
        NS *= 2
    capN = (NS * 2) // 3
    n = 256
    while n < ne and n < NS:
        n *= 2
    if ne > 256 and cut > 0:
        counts = np.bincount(weight_bins(w, min_weight), minlength=1024)[::-1]     # from the top bin down
        above = np.cumsum(counts)
        t = int(np.argmax(above >= cut))                                           # the threshold bin
        cnt, crowd = int(above[t]), int(counts[:t + 1].max())
        if cnt <= capN and crowd <= 512:
            return ("ranked" if ne <= 2048 else "ranked-rounds"), ne, 0
        if ne > 1024 and cnt <= NS:
            n = 256
            while n < cnt:
                n *= 2
            return "one-pass", ne, n
    if ne <= 256:
        return "registers", ne, n
    return ("passes" if ne <= n else "passes-refill"), ne, n


def run_deciders(w, max_quantity, min_weight=MIN_WEIGHT):
    """how the order of the neighbours among the kept rows is decided where the sort words (prune_pack32: 32 - sbits key bits,
    then the slot) agree in the key: 'lds' (the 32 weight bits behind the key), 'weight' (the full weight) or 'index' (bit-equal
    weights: the canonical index) — the set of those that occur"""
    w = np.asarray(w, np.float64)
    w = w[w >= min_weight]
    ne, cut = len(w), min(int(max_quantity), len(w))
    sbits = 1
    while (1 << sbits) < ne:
        sbits += 1
    kept = w[np.argsort(-w, kind="stable")][:cut]
    body = kept.view(np.uint64) << np.uint64(1)
    key = body >> np.uint64(64 - (32 - sbits))
    nxt = ((body << np.uint64(32 - sbits)) >> np.uint64(32))
    same = key[1:] == key[:-1]
    kinds = set()
    if np.any(same & (nxt[1:] != nxt[:-1])):
        kinds.add("lds")
    if np.any(same & (nxt[1:] == nxt[:-1]) & (kept[1:] != kept[:-1])):
        kinds.add("weight")
    if np.any(kept[1:] == kept[:-1]):
        kinds.add("index")
    return kinds


def far_apart(w, max_quantity):
    """the weights on a plane grid 5 m wide (covariance 0.01 I): nothing merges, PruneModel's output is the sorted cut itself"""
    n = len(w)
    side = int(np.ceil(np.sqrt(n)))
    gx, gy = np.meshgrid(np.arange(side) * 5.0, np.arange(side) * 5.0)
    return Case(w, np.column_stack([gx.ravel()[:n], gy.ravel()[:n], np.zeros(n)]), iso(n), max_quantity)


def one_bin(rng, n, lo=1.0):
    """n distinct weights in one histogram bin, [lo, lo (1 + 1 / 32)), shuffled"""
    return lo * (1.0 + rng.permutation(n) * (1.0 / 32 / (n + 1)))


def with_ties(rng, w):
    """the three heaviest weights once more: one bit-equal, one a unit in the last place lighter — the full weight and the
    canonical index decide between neighbours — and the whole shuffled"""
    top = np.sort(w)[-3:]
    w = np.concatenate([w, top, np.nextafter(top, 0.0)])
    return w[rng.permutation(len(w))]


def order_case(name):
    """(case, branch its weights take, run deciders that must occur): the smallest maps that reach each branch of phase A"""
    rng = np.random.default_rng(sum(name.encode()))
    if name in ("registers-256", "ranked-257", "ranked-2048", "ranked-rounds-2049"):
        n = int(name.rsplit("-", 1)[1])
        w = weights(rng, n - 6)
        return far_apart(with_ties(rng, w), 600), name.rsplit("-", 1)[0], set()
    if name == "one-pass":        # 400 in the threshold bin (more than capN = 341, no more than NS = 512), 700 lighter
        w = np.concatenate([one_bin(rng, 394), weights(rng, 700, 0.01, 0.9)])
        return far_apart(with_ties(rng, w), 40), "one-pass", {"lds", "weight", "index"}
    if name == "passes":          # 400 in one bin: ranked refused, one pass of 512
        return far_apart(with_ties(rng, one_bin(rng, 394)), 40), "passes", {"lds", "weight", "index"}
    if name == "passes-refill":   # 600 in one bin: more than the sort width, the worse half refilled
        return far_apart(with_ties(rng, one_bin(rng, 594)), 40), "passes-refill", {"lds", "weight", "index"}
    raise KeyError(name)


ORDER_IDS = ["registers-256", "ranked-257", "ranked-2048", "ranked-rounds-2049", "one-pass", "passes", "passes-refill"]
