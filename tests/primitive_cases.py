"""Inputs, references and bounds for the device arithmetic primitives (monorfs_amd/csrc/phd_primitives_test.h): for
every op the seeded input generator, the reference — Python integers and `fractions.Fraction` where the result is
rational, mpmath at 200 bits (60 digits) otherwise, a numpy transcription of the stated ORDER where the claim is bit
equality — and the bound with its derivation. Nothing here needs a GPU.

A check takes `run(op, in_array, out_dtype, out_count) -> numpy array`: `Navigator.test_primitive` on the device
(tests/test_gpu_primitives.py) or the host transcription tests/primitive_refs_check.cpp (tests/test_primitive_refs.py), which
shows that the references stay inside their own bounds before a GPU is asked. A check asserts on every input it
generates (nothing is filtered out) and returns what it measured."""
import functools
import math
import os
import re
from fractions import Fraction

import mpmath
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
mp = mpmath.mp
mp.prec = 200

# ---- the powers of the unit roundoff, stated once -------------------------------------------------------------------------
U = 2.0 ** -53                    # unit roundoff of a double: one rounding to nearest is a relative (1 + d), |d| <= U
ULP = 2.0 ** -52                  # the spacing of doubles in [1, 2)
U_F = Fraction(1, 2 ** 53)
TINY = 2.0 ** -1074               # the smallest subnormal
MIN_NORMAL = 2.0 ** -1022
LN2_256 = mp.log(2) / 256

# exp_neg, a normal result: T[j] within 1 ulp of 2^(j/256) (checked on its own, check_exp_table), the polynomial's last
# fused multiply-add, the product t * p, the truncation r^5 / 120 of the degree-4 Taylor polynomial at |r| <= ln 2 / 512
# (relative (1.354e-3)^5 / 120 = 3.8e-17), the two-constant reduction and the earlier steps of the Horner chain, whose
# roundings reach the result scaled by |r| (1e-18 together). A subnormal result adds ldexp's second rounding, TINY.
E_NEG = ULP + U + U + 4e-17 + 1e-18
# exp_pair: the degree-3 polynomial drops r^4 / 24; ln 2 / 256 as one constant is off by at most 2.2e-19, times
# n = 369.33 |x|, an absolute error of the reduced argument and so a relative one of the result; then the same roundings
E_PAIR_TRUNC = float((mp.log(2) / 512) ** 4 / 24)
E_PAIR_SLOPE = 2.2e-19 * 369.33


def e_pair(x):
    return E_PAIR_TRUNC + E_PAIR_SLOPE * np.abs(x) + E_NEG


# AccurateDWPlusDW and DWPlusFP (Joldes, Muller, Popescu: Tight and rigorous error bounds for basic building blocks of
# double-word arithmetic, ACM TOMS 44, 2017: Theorems 3.1 and 2.2), normalised inputs, no underflow
E_DD_ADD = 3 * U_F ** 2 + 13 * U_F ** 3
E_DD_ADD_D = 2 * U_F ** 2
# dd_wave_scan over 64 lanes: six levels of dd_add on non-negative numbers; each level's result is within (1 + E_DD_ADD) of
# the exact sum of its two operands, which carry the levels before
E_DD_SCAN = (1 + E_DD_ADD) ** 6 - 1
# gauss_logw: d = x - m rounds once per coordinate (every term G_ij d_i d_j carries two of them), the longest chain of the
# evaluation is six fused operations deep (g[3] d0 -> fma -> fma -> t0 d0 .. three fused additions): (1 + d)^9, gamma_9
GAMMA9 = 9 * U_F / (1 - 9 * U_F)


def op_numbers():
    """{name: number} of the PT_ enumeration of phd_primitives_test.h (the header is the one statement of it)"""
    text = open(os.path.join(ROOT, "monorfs_amd", "csrc", "phd_primitives_test.h")).read()
    body = re.search(r"enum \{(.*?)\};", text, re.S).group(1)
    names = [t.split("=")[0].strip() for t in body.replace("\n", " ").split(",")]
    assert names[0] == "PT_EXP_NEG" and "= 1" in body
    return {n: k + 1 for k, n in enumerate(names)}


OP = op_numbers()
f8, u8, i8, i4 = np.float64, np.uint64, np.int64, np.int32


def bits(x):
    return np.ascontiguousarray(x, f8).view(u8)


def frac(x):
    return Fraction(float(x))


def to_mpf(q):
    return mp.mpf(q.numerator) / mp.mpf(q.denominator)


def nearest_double(q):
    """the double nearest to the Fraction q (ties to even; int / int is correctly rounded in Python)"""
    return q.numerator / q.denominator


# ==== exp_neg / exp_pair ==============================================================================================
@functools.lru_cache(maxsize=None)
def exp_inputs():
    rng = np.random.default_rng(0xE4B0)
    parts = [rng.uniform(-745, 0, 30000), rng.uniform(-40, 0, 25000), rng.uniform(0, 40, 15000), rng.uniform(-1e-3, 1e-3, 10000)]
    # both neighbours of (and the double nearest to) the reduction boundaries (k + 1/2) ln 2 / 256: the largest |r|, the ties of rint
    ks = np.unique(np.concatenate([rng.integers(-275200, 14780, 4000), np.arange(-4, 4), [-275200, -261600, -261500, 14779]]))
    b = np.array([float((int(k) + mp.mpf(0.5)) * LN2_256) for k in ks])
    parts += [b, np.nextafter(b, -np.inf), np.nextafter(b, np.inf)]
    parts.append(np.array([0.0, -0.0, 5e-324, -5e-324, 1e-323, -1e-323, 2.0 ** -1022, -2.0 ** -1022, 700.0, -708.3, -708.5, -745.1, -745.2, -800.0,
                           np.nextafter(-800.0, 0), np.nextafter(-800.0, -np.inf), -1000.0, -np.inf, np.nan]))
    x = np.concatenate(parts)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def exp_reference():
    """exp(x) for the finite x of exp_inputs with x >= -800: (hi, lo) with hi + lo = exp(x) to 1e-32 where the result is
    normal (lo = 0 elsewhere), and {index: mpf} for the results below 2^-1000, which are compared in mpmath"""
    x = exp_inputs()
    hi, lo, small = np.zeros(len(x)), np.zeros(len(x)), {}
    for k in np.nonzero(np.isfinite(x) & (x >= -800))[0]:
        r = mp.exp(mp.mpf(float(x[k])))
        if x[k] < -690:
            small[int(k)] = r
        else:
            hi[k] = float(r)
            lo[k] = float(r - mp.mpf(hi[k]))
    hi.setflags(write=False)
    lo.setflags(write=False)
    return hi, lo, small


def check_exp(run, pair):
    """exp_neg (pair = False) or exp_pair with keep = true on exp_inputs. Returns (largest relative error of a normal result,
    the x it occurred at, the largest error over the bound)."""
    x = exp_inputs()
    hi, lo, small = exp_reference()
    if pair:
        rec = np.zeros((len(x), 2), u8)
        rec[:, 0], rec[:, 1] = bits(x), 1
        y = run(OP["PT_EXP_PAIR"], rec, f8, len(x))
        bound = e_pair(np.maximum(x, -800.0))
    else:
        y = run(OP["PT_EXP_NEG"], x, f8, len(x))
        bound = np.full(len(x), E_NEG)
    yb = bits(y)
    zero = (x < -800) | np.isnan(x) if pair else (x < -800)          # exactly +0: below -800, -inf; exp_pair: a NaN too
    assert np.all(yb[zero] == 0), "not exactly +0: x = %r" % (x[zero][yb[zero] != 0][:5],)
    if not pair:
        assert np.all(np.isnan(y[np.isnan(x)])), "exp_neg(NaN) is not a NaN"
    normal = hi > 0
    assert np.count_nonzero(normal) + len(small) + np.count_nonzero(x < -800) + np.count_nonzero(np.isnan(x)) == len(x)
    with np.errstate(invalid="ignore", over="ignore"):
        # (y - hi is exact for any y within a factor two of hi; a y further off fails whatever the subtraction rounds to)
        rel = np.abs((y[normal] - hi[normal]) - lo[normal]) / hi[normal]
    rel = np.where(np.isnan(rel), np.inf, rel)
    worst = int(np.argmax(rel / bound[normal]))
    at = np.nonzero(normal)[0]
    assert np.all(rel <= bound[normal]), "%d normal results outside the bound; worst at x = %r: relative %.4g, bound %.4g" % (
        np.count_nonzero(rel > bound[normal]), x[at[worst]], rel[worst], bound[normal][worst])
    for k, r in small.items():          # results near and below the subnormal range; where subnormal, ldexp rounds a second time
        err = abs(mp.mpf(float(y[k])) - r) if np.isfinite(y[k]) else mp.inf
        assert err <= float(bound[k]) * r + (TINY if r < MIN_NORMAL else 0.0), "x = %r: %r, reference %s" % (x[k], y[k], mp.nstr(r, 20))
    top = int(np.argmax(rel))
    return float(rel[top]), float(x[at[top]]), float(rel[worst] / bound[normal][worst])


def check_exp_pair_dropped(run):
    """keep = false: +0 for every input, NaN included"""
    x = exp_inputs()
    rec = np.zeros((len(x), 2), u8)
    rec[:, 0] = bits(x)
    y = run(OP["PT_EXP_PAIR"], rec, f8, len(x))
    assert np.all(bits(y) == 0), "exp_pair(x, keep = false) != +0 at x = %r" % (x[bits(y) != 0][:5],)


@functools.lru_cache(maxsize=None)
def exp_table_reference():
    """2^(j/256) correctly rounded, j = 0 .. 255"""
    return np.array([float(mp.power(2, mp.mpf(j) / 256)) for j in range(256)])


def check_exp_table(run):
    """every entry within 1 ulp of 2^(j/256): the premise of E_NEG. Returns the largest error in ulps."""
    t = run(OP["PT_EXP_TAB"], np.zeros(0, f8), f8, 256)
    worst = 0.0
    for j in range(256):
        exact = mp.power(2, mp.mpf(j) / 256)
        ulp = math.ulp(float(exact)) if j else ULP
        err = float(abs(mp.mpf(float(t[j])) - exact) / ulp)
        assert err <= 1.0, "T[%d] = %r is %.3f ulp from 2^(%d/256)" % (j, t[j], err, j)
        worst = max(worst, err)
    assert t[0] == 1.0
    return worst


# ==== gauss_record / gauss_logw =======================================================================================
def _rotations(rng, n):
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], 1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], 1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1)], 1)


TRI = ([0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2])


@functools.lru_cache(maxsize=None)
def gauss_inputs():
    """(w, m[3], Pi[6], mult, x[3]) of N components and a point each: a third well conditioned (eigenvalues within a factor
    100), a third of condition 1e12, a third of either kind 2 km from the origin; the point 0 .. 40 standard deviations
    (Mahalanobis) from the mean in a random direction, every fifth ON the mean"""
    n = 3 * 1025
    rng = np.random.default_rng(0x6A55)
    V = _rotations(rng, n)
    s = 10.0 ** rng.uniform(-4, 0, n)
    lam = s[:, None] * 10.0 ** rng.uniform(0, 2, (n, 3))
    ill = np.arange(n) % 3 == 1
    ill |= (np.arange(n) % 3 == 2) & (rng.random(n) < 0.5)
    lam[ill] = s[ill, None] * np.array([1.0, 1e-6, 1e-12]) * 10.0 ** rng.uniform(0, 0.3, (np.count_nonzero(ill), 3))
    P = np.einsum("nij,nj,nkj->nik", V, lam, V)
    Pinv = np.einsum("nij,nj,nkj->nik", V, 1.0 / lam, V)
    m = rng.uniform(-5, 5, (n, 3))
    far = np.arange(n) % 3 == 2
    m[far] += 2000.0 * V[far, :, 0]
    k = rng.uniform(0, 40, n)
    dirn = rng.normal(size=(n, 3))
    dirn /= np.linalg.norm(dirn, axis=1, keepdims=True)
    x = m + np.einsum("nij,nj->ni", V, np.sqrt(lam) * dirn * k[:, None])
    x[::5] = m[::5]
    w = 10.0 ** rng.uniform(-3, 0.3, n)
    mult = 0.15915494309189535 / np.sqrt(np.prod(lam, axis=1))
    out = (w, m, Pinv[:, TRI[0], TRI[1]].copy(), mult, x)
    for a in out:
        a.setflags(write=False)
    assert np.linalg.cond(P[ill]).min() > 1e11 and np.linalg.cond(P[~ill]).max() < 1e3
    return out


def numpy_gauss_record(w, m, Pi, mult):
    g = np.zeros((len(w), 10))
    g[:, 0:3] = m
    g[:, 3], g[:, 4], g[:, 5] = -0.5 * Pi[:, 0], -Pi[:, 1], -Pi[:, 2]
    g[:, 6], g[:, 7], g[:, 8] = -0.5 * Pi[:, 3], -Pi[:, 4], -0.5 * Pi[:, 5]
    g[:, 9] = np.log(w * mult)
    return g


def check_gauss_record(run):
    w, m, Pi, mult, _ = gauss_inputs()
    n = len(w)
    rec = np.concatenate([w[:, None], m, Pi, mult[:, None]], axis=1)
    g = run(OP["PT_GAUSS_RECORD"], rec, f8, n * 10).reshape(n, 10)
    want = numpy_gauss_record(w, m, Pi, mult)
    assert np.array_equal(bits(g[:, :9]), bits(want[:, :9])), "entries 0 .. 8 are not -Pi / 2, -Pi and m bit for bit"
    worst = 0.0
    for k in range(n):
        exact = mp.log(mp.mpf(float(w[k])) * mp.mpf(float(mult[k])))
        err, tol = abs(mp.mpf(float(g[k, 9])) - exact), ULP * abs(exact) + ULP      # the product's rounding (absolute U in the log) and the log's own ulp
        assert err <= tol, "g9 of record %d: %r, log(w mult) = %s" % (k, g[k, 9], mp.nstr(exact, 20))
        worst = max(worst, float(err / tol))
    return worst


@functools.lru_cache(maxsize=None)
def gauss_logw_reference():
    """per record: the exact g9 + sum G_ij d_i d_j with d = x - m exact, and the sum of the absolute values (Fractions)"""
    w, m, Pi, mult, x = gauss_inputs()
    g = numpy_gauss_record(w, m, Pi, mult)
    exact, mag = [], []
    for k in range(len(w)):
        d = [frac(x[k, t]) - frac(m[k, t]) for t in range(3)]
        G = [frac(v) for v in g[k, 3:9]]
        terms = [G[0] * d[0] * d[0], G[1] * d[0] * d[1], G[2] * d[0] * d[2], G[3] * d[1] * d[1], G[4] * d[1] * d[2], G[5] * d[2] * d[2]]
        exact.append(frac(g[k, 9]) + sum(terms))
        mag.append(abs(frac(g[k, 9])) + sum(abs(t) for t in terms))
    return g, exact, mag


def check_gauss_logw(run):
    """gauss_logw against the exact value with the condition-aware bound GAMMA9 * (|g9| + sum |G_ij d_i d_j|), and the composed
    density exp_pair(gauss_logw) against exp of the exact exponent with |dlogw| + E_PAIR. Returns the largest error over its bound
    of each."""
    _, _, _, _, x = gauss_inputs()
    g, exact, mag = gauss_logw_reference()
    n = len(g)
    out = run(OP["PT_GAUSS_LOGW"], np.concatenate([g, x], axis=1), f8, 2 * n).reshape(n, 2)
    worst_l = worst_d = 0.0
    for k in range(n):
        assert np.isfinite(out[k, 0]), "record %d: logw = %r" % (k, out[k, 0])
        dl = GAMMA9 * mag[k]
        err = abs(frac(out[k, 0]) - exact[k])
        assert err <= dl, "record %d: logw %r, exact %.17g, error %.3g > %.3g" % (k, out[k, 0], float(exact[k]), float(err), float(dl))
        if dl:
            worst_l = max(worst_l, float(err / dl))
        ref = mp.exp(to_mpf(exact[k]))
        tol = (float(dl) + float(e_pair(max(float(out[k, 0]), -800.0)))) * ref + (TINY if ref < MIN_NORMAL else 0.0)
        derr = abs(mp.mpf(float(out[k, 1])) - ref)
        assert derr <= tol, "record %d: density %r, exact %s (logw %r)" % (k, out[k, 1], mp.nstr(ref, 20), out[k, 0])
        worst_d = max(worst_d, float(derr / tol))
    return worst_l, worst_d


# ==== double-double helpers ===========================================================================================
def _magnitudes(rng, n):
    return rng.choice([-1.0, 1.0], n) * rng.uniform(1, 2, n) * 2.0 ** rng.integers(-60, 61, n)


def _with_low(rng, hi):
    """double-doubles (hi, lo) with hi = fl(hi + lo): lo up to half an ulp of hi, either sign, some zero"""
    n = len(hi)
    lo = hi * rng.uniform(-1, 1, n) * U * rng.choice([0.0, 1.0, 2.0 ** -20], n)
    s = hi + lo
    return s, lo - (s - hi)


def _normalised(rng, n, positive=False):
    hi = _magnitudes(rng, n)
    return _with_low(rng, np.abs(hi) if positive else hi)


def two_sum_inputs():
    rng = np.random.default_rng(0xDD01)
    a, b = _magnitudes(rng, 6000), _magnitudes(rng, 6000)
    b[:1500] = a[:1500] * rng.uniform(-2, 2, 1500)                       # close magnitudes: the sum's low part is long
    b[1500:2000] = -a[1500:2000] * (1 + rng.integers(-4, 5, 500) * ULP)    # cancellation
    sw = (np.abs(a) > np.abs(b)) & (rng.random(6000) < 0.7)              # mostly |a| < |b|: the order dd_quick could not take
    a[sw], b[sw] = b[sw], a[sw]
    assert np.count_nonzero(np.abs(a) < np.abs(b)) > 3000
    return a, b


def check_two_sum(run, quick):
    a, b = two_sum_inputs()
    if quick:
        sw = np.abs(a) < np.abs(b)
        a, b = np.where(sw, b, a), np.where(sw, a, b)
    r = run(OP["PT_DD_QUICK" if quick else "PT_DD_TWO_SUM"], np.stack([a, b], 1), f8, 2 * len(a)).reshape(-1, 2)
    assert np.array_equal(bits(r[:, 0]), bits(a + b)), "hi != fl(a + b)"
    for k in range(len(a)):
        assert frac(r[k, 0]) + frac(r[k, 1]) == frac(a[k]) + frac(b[k]), "hi + lo != a + b at a = %r, b = %r: %r" % (a[k], b[k], r[k])


def check_two_sum_of_product(run):
    """dd_two_sum(a * b, c) with the product formed by the caller, where contraction is on: hi = fl(fl(a b) + c) and hi + lo =
    fl(a b) + c only while the helper's own `fp contract(off)` keeps its first addition from fusing with the product. (The
    additions of dd_add take sums alone: nothing outside it can make its pragma observable.)"""
    rng = np.random.default_rng(0xDD05)
    a, b = _magnitudes(rng, 4000), _magnitudes(rng, 4000)
    p = a * b
    c = np.where(rng.random(4000) < 0.5, -p * (1 + rng.integers(-8, 9, 4000) * ULP), p * rng.uniform(-2, 2, 4000))
    fused = np.array([nearest_double(frac(a[k]) * frac(b[k]) + frac(c[k])) for k in range(4000)])
    assert np.count_nonzero(fused != p + c) > 1000, "the inputs do not tell a fused first addition from a rounded product"
    r = run(OP["PT_DD_TWO_SUM_PROD"], np.stack([a, b, c], 1), f8, 8000).reshape(-1, 2)
    assert np.array_equal(bits(r[:, 0]), bits(p + c)), "hi != fl(fl(a b) + c): %d of 4000 (the first addition fused with the product?)" % np.count_nonzero(r[:, 0] != p + c)
    for k in range(4000):
        assert frac(r[k, 0]) + frac(r[k, 1]) == frac(p[k]) + frac(c[k]), "hi + lo != fl(a b) + c at record %d" % k


def dd_add_inputs():
    rng = np.random.default_rng(0xDD02)
    n = 6000
    xh, xl = _normalised(rng, n)
    yh = _magnitudes(rng, n)
    yh[:1500] = xh[:1500] * rng.uniform(-2, 2, 1500)                                    # overlapping operands, both signs
    yh[1500:2000] = -xh[1500:2000] * (1 + rng.integers(-3, 4, 500) * ULP)                 # the high parts cancel
    yh, yl = _with_low(rng, yh)
    assert np.array_equal(yh, yh + yl) and np.array_equal(xh, xh + xl)
    return xh, xl, yh, yl


def _assert_dd_close(r, exact, eps, what):
    """|hi + lo - exact| <= eps |exact| for every row, in Fractions; returns the largest error over the bound"""
    worst = Fraction(0)
    for k in range(len(r)):
        assert np.isfinite(r[k]).all(), "%s %d: %r" % (what, k, r[k])
        err, tol = abs(frac(r[k, 0]) + frac(r[k, 1]) - exact[k]), eps * abs(exact[k])
        assert err <= tol, "%s %d: (%r, %r), exact %.17g: relative %.4g > %.4g" % (what, k, r[k, 0], r[k, 1], float(exact[k]), float(err / abs(exact[k])), float(eps))
        if tol:
            worst = max(worst, err / tol)
    return float(worst)


def check_dd_add(run):
    xh, xl, yh, yl = dd_add_inputs()
    r = run(OP["PT_DD_ADD"], np.stack([xh, xl, yh, yl], 1), f8, 2 * len(xh)).reshape(-1, 2)
    exact = [frac(xh[k]) + frac(xl[k]) + frac(yh[k]) + frac(yl[k]) for k in range(len(xh))]
    return _assert_dd_close(r, exact, E_DD_ADD, "dd_add")


def check_dd_add_d(run):
    xh, xl, yh, _ = dd_add_inputs()
    r = run(OP["PT_DD_ADD_D"], np.stack([xh, xl, yh], 1), f8, 2 * len(xh)).reshape(-1, 2)
    exact = [frac(xh[k]) + frac(xl[k]) + frac(yh[k]) for k in range(len(xh))]
    return _assert_dd_close(r, exact, E_DD_ADD_D, "dd_add_d")


def resample_weights(P, rng):
    """weight vectors of the kind tests/test_gpu_resample.py draws: random^6, nine tenths zero, alternating 1 and 1e-12"""
    w = rng.random(P) ** 6
    out = [w / w.sum()]
    w = rng.random(P) * (rng.random(P) < 0.1)
    w[rng.integers(P)] += 1e-3
    out.append(w / w.sum())
    w = np.where(np.arange(P) % 2 == 0, 1.0, 1e-12)
    out.append(w / w.sum())
    return out


def dd_scan_inputs():
    """waves of 64 non-negative double-doubles: resampling weights (low part 0, as k_nr_stats scans them), chunk sums with a low
    part, mixed magnitudes over 120 binades, zeros"""
    rng = np.random.default_rng(0xDD03)
    hi = np.concatenate(resample_weights(256, rng) + [np.abs(_magnitudes(rng, 256))])
    lo = np.zeros(len(hi))
    h2, l2 = _normalised(rng, 512, positive=True)
    h2[::7], l2[::7] = 0.0, 0.0
    h2[256:] *= 2.0 ** -40
    l2[256:] *= 2.0 ** -40
    return np.concatenate([hi, h2]), np.concatenate([lo, l2])


def check_dd_scan(run, width):
    """lane l of a wave holds the sum of lanes max(0, l - width + 1) .. l (width 64: the prefix sum; 16: what the shuffles leave
    in the lanes beyond the first 16, which the callers do not read)"""
    hi, lo = dd_scan_inputs()
    n = len(hi)
    assert n % 256 == 0
    r = run(OP["PT_DD_SCAN_64" if width == 64 else "PT_DD_SCAN_16"], np.stack([hi, lo], 1), f8, 2 * n).reshape(-1, 2)
    v = [frac(hi[k]) + frac(lo[k]) for k in range(n)]
    exact = [sum(v[max(k - k % 64, k - width + 1):k + 1]) for k in range(n)]
    return _assert_dd_close(r, exact, E_DD_SCAN, "dd_wave_scan(width %d) lane" % width)


def slot_target_inputs():
    rng = np.random.default_rng(0xDD04)
    rows = []
    for P in (1, 2, 3, 1000, 17409, 65536):
        invP = 1.0 / P
        for u in (0.0, 2.0 ** -60, 0.37, 1.0 - U):
            idx = sorted({0, min(1, P - 1), P - 1} | set(int(t) for t in rng.integers(0, P, 24)))
            rows += [(i, u / P, invP) for i in idx]
    return rows


def check_slot_target(run):
    rows = slot_target_inputs()
    rec = np.zeros((len(rows), 3), u8)
    rec[:, 0] = np.array([r[0] for r in rows], i8).view(u8)
    rec[:, 1], rec[:, 2] = bits([r[1] for r in rows]), bits([r[2] for r in rows])
    r = run(OP["PT_SLOT_TARGET"], rec, f8, 2 * len(rows)).reshape(-1, 2)
    exact = [frac(R0) + i * frac(invP) for i, R0, invP in rows]
    return _assert_dd_close(r, exact, E_DD_ADD_D, "slot_target")     # i * invP is exact in (ph, pl); then one DWPlusFP


# ==== small_div =======================================================================================================
def small_div_divisors():
    rng = np.random.default_rng(0x5D17)
    return np.array([1, 2, 3, 5, 7, 255, 256, 257, 1000, 4095, 4097, 65535, 65536, 2 ** 23 - 1, 2 ** 24 - 1] + [int(d) for d in rng.integers(1, 2 ** 24, 32)], i4)


def check_small_div(run):
    """the sweep runs where small_div does: every s in [0, 2^24) against each d, compared with s / d there"""
    d = small_div_divisors()
    r = run(OP["PT_SMALL_DIV"], d, u8, 2 * len(d)).reshape(-1, 2)
    bad = [(int(d[k]), int(r[k, 0]), 2 ** 24 - int(r[k, 1])) for k in range(len(d)) if r[k, 0] or r[k, 1]]
    assert not bad, "small_div(s, d) != s / d: (d, mismatches, first s) = %r" % (bad[:8],)


# ==== weight bins =====================================================================================================
M64 = (1 << 64) - 1


def py_bin_base(minw):
    return ((int(bits([minw])[0]) << 1) & M64) >> 48


def py_bin_of_bits(b, base):
    return min(max((((int(b) << 1) & M64) >> 48) - base, 0), 1023)


def py_prune_key(w):
    b = int(bits([w])[0])
    return (~b & M64) if b >> 63 else (b | (1 << 63))


def bin_min_weights():
    import paramspace
    from monorfs_amd.abi import prm3d_defaults
    out = [prm3d_defaults(1, 600, 8).min_weight]
    out += [paramspace.SETS[name]["min_weight"] for name in ("small_minw", "small_minw_wide", "large_minw")]
    return out


def bin_weights(minw):
    """positive weights around the 1024 bins counted from MinWeight's: 40 binades below to 40 above, bin edges and their
    neighbours, subnormals, 0, the largest double and +inf; ascending"""
    rng = np.random.default_rng(0xB175)
    w = minw * 2.0 ** rng.uniform(-40, 40, 3000)
    e = minw * 2.0 ** rng.integers(-3, 34, 200) * (1 + rng.integers(0, 32, 200) / 32.0)
    w = np.concatenate([w, e, np.nextafter(e, 0), np.nextafter(e, np.inf), minw * 2.0 ** np.array([16.0, 17.0, 31.0, 32.0, 33.0]),
                        [0.0, 5e-324, 2.0 ** -1060, np.nextafter(MIN_NORMAL, 0), MIN_NORMAL, minw, np.nextafter(minw, 0), np.finfo(f8).max, np.inf]])
    return np.sort(w)


def check_weight_bins(run, minw):
    head = bits([minw])
    e = run(OP["PT_BIN_EDGE"], head, u8, 1024)
    base = py_bin_base(minw)
    assert int(e[0]) == base, "weight_bin_base(%r) = %d, from the bit pattern %d" % (minw, e[0], base)
    assert [int(v) for v in e[1:]] == [(base + b) << 47 for b in range(1, 1024)], "weight_bin_edge differs from (base + b) << 47"
    edges = e[1:].view(f8)
    assert np.all(np.diff(edges) > 0) and py_bin_of_bits(bits([minw])[0], base) == 0 and edges[0] > minw and minw * 33 >= edges[0] * 32
    below = np.nextafter(edges, 0)
    w = bin_weights(minw)
    allw = np.concatenate([edges, below, w])
    got = run(OP["PT_BIN_OF_BITS"], np.concatenate([head, bits(allw)]), i4, len(allw))
    assert np.array_equal(got, [py_bin_of_bits(b, base) for b in bits(allw)]), "weight_bin_of_bits differs from the integer arithmetic"
    assert np.array_equal(got[:1023], np.arange(1, 1024)), "bin(edge(b)) != b"
    assert np.array_equal(got[1023:2046], np.arange(0, 1023)), "the double below edge(b) is not in bin b - 1"
    gw = got[2046:]
    assert np.all(np.diff(gw) >= 0), "not monotone in the weight"
    assert np.all(gw[w < edges[0]] == 0) and np.all(gw[w >= edges[-1]] == 1023) and gw[-1] == 1023 and np.isinf(w[-1]) and gw[0] == 0
    assert np.all(gw[w >= minw * 2.0 ** 33] == 1023) and 0 < gw[np.searchsorted(w, minw * 2.0 ** 16)] < 1023
    key = run(OP["PT_BIN_OF_KEY"], np.concatenate([head, bits(allw)]), i4, len(allw))
    assert np.array_equal(key, got), "the bin of a prune_key differs from the bin of the double's own pattern"
    assert [py_bin_of_bits(py_prune_key(v), base) for v in allw[::37]] == [int(v) for v in got[::37]]


# ==== fixed-order reductions and scans ================================================================================
def order_sensitive(n, seed):
    """doubles whose sum depends on the order of the additions: magnitudes over 30 binades, both signs"""
    rng = np.random.default_rng(seed)
    v = rng.choice([-1.0, 1.0], n) * rng.uniform(1, 2, n) * 2.0 ** rng.integers(-15, 16, n)
    return v


def numpy_wave_sum(v):
    """xor butterfly 32, 16, ..., 1 on waves of 64: every lane's value"""
    v = np.array(v, f8).reshape(-1, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lane ^ o]
    return v.reshape(-1)


def numpy_block_sum(v, block):
    """block_sum_1024: wave butterflies, then t = 0; t += total of wave 0, 1, ... in order"""
    tot = numpy_wave_sum(v).reshape(-1, block // 64, 64)[:, :, 0]
    t = np.zeros(len(tot))
    for q in range(block // 64):
        t = t + tot[:, q]
    return np.repeat(t, block)


def numpy_block_tree_sum(v):
    """block_tree_sum: x[l] = (r[l] + r[l + 128]) + (r[l + 64] + r[l + 192]) for l < 64, then x += shfl_down(x, s) for
    s = 32, 16, ..., 1 (a lane whose source lies beyond the wave reads itself); lane 0's value, to every thread"""
    r = np.array(v, f8).reshape(-1, 256)
    x = (r[:, 0:64] + r[:, 128:192]) + (r[:, 64:128] + r[:, 192:256])
    lane = np.arange(64)
    for s in (32, 16, 8, 4, 2, 1):
        x = x + x[:, np.where(lane + s < 64, lane + s, lane)]
    return np.repeat(x[:, 0], 256)


def check_sums(run):
    v = order_sensitive(2048, 0x50A1)
    assert np.array_equal(bits(run(OP["PT_WAVE_SUM"], v, f8, len(v))), bits(numpy_wave_sum(v))), "wave_sum: not the xor butterfly 32 .. 1"
    for name, block in (("PT_BLOCK_SUM_256T", 256), ("PT_BLOCK_SUM_512", 512), ("PT_BLOCK_SUM_1024", 1024)):
        assert np.array_equal(bits(run(OP[name], v, f8, len(v))), bits(numpy_block_sum(v, block))), "block_sum_1024 at %d threads" % block
    assert np.array_equal(bits(run(OP["PT_BLOCK_TREE_SUM"], v, f8, len(v))), bits(numpy_block_tree_sum(v))), "block_tree_sum"
    s4 = order_sensitive(4 * 999, 0x50A2).reshape(-1, 4)
    got = run(OP["PT_BLOCK_SUM_256"], s4, f8, len(s4))
    assert np.array_equal(bits(got), bits(((s4[:, 0] + s4[:, 1]) + s4[:, 2]) + s4[:, 3])), "block_sum_256: not ((s0 + s1) + s2) + s3"
    # the orders are told apart by the data: the butterfly, the sequential sum and the reversed pairing differ on these vectors
    seq = np.array([math.fsum(w) for w in v.reshape(-1, 64)])
    assert np.any(numpy_wave_sum(v).reshape(-1, 64)[:, 0] != seq)
    up = np.array(v, f8).reshape(-1, 64)
    for o in (1, 2, 4, 8, 16, 32):
        up = up + up[:, np.arange(64) ^ o]
    assert np.any(up.reshape(-1) != numpy_wave_sum(v)), "the vector does not tell the butterfly 32 .. 1 from 1 .. 32"
    assert np.any(((s4[:, 0] + s4[:, 1]) + s4[:, 2]) + s4[:, 3] != (s4[:, 0] + s4[:, 1]) + (s4[:, 2] + s4[:, 3]))


def check_extrema(run):
    """wave_max / wave_min: the butterfly 32 .. 1 of fmax / fmin, which for numbers is the wave's extremum in every lane
    (infinities included; no NaN and no zeros of both signs, where fmax is not one function)"""
    v = order_sensitive(1024, 0x50A3)
    v[64:128] = np.abs(v[64:128])
    v[130], v[200], v[260] = np.inf, -np.inf, -np.inf
    v[320:384] = -np.inf
    for name, f in (("PT_WAVE_MAX", np.max), ("PT_WAVE_MIN", np.min)):
        want = np.repeat(f(v.reshape(-1, 64), axis=1), 64)
        assert np.array_equal(bits(run(OP[name], v, f8, len(v))), bits(want)), name


def check_incl_scan(run):
    rng = np.random.default_rng(0x50A4)
    v = rng.integers(-1000, 1000, 1024).astype(i4)
    v[0:64] = 0
    v[64:128] = 1
    v[128:192] = rng.integers(0, 2, 64)
    v[192:256] = 2 ** 25 - 1                       # (64 of them: 2^31 - 64, the largest total an int holds)
    want = np.cumsum(v.reshape(-1, 64), axis=1, dtype=i8).astype(i4).reshape(-1)
    assert np.array_equal(run(OP["PT_WAVE_INCL_SCAN"], v, i4, len(v)), want)
    assert want[127] == 64 and want[63] == 0 and want[255] == 2 ** 31 - 64


def check_first_max(run):
    """(m, lane): the largest v among the lanes with `has` (the others bring -inf) and the smallest lane that holds it;
    (-inf, 0) when no lane has one"""
    rng = np.random.default_rng(0x50A5)
    waves = []

    def wave(v, has):
        waves.append((np.where(has, v, -np.inf), has))
    base = rng.random(64)
    for at in (0, 63, 17):                                              # a unique maximum: in lane 0, in lane 63, inside
        v = base.copy()
        v[at] = 2.0
        wave(v, np.ones(64, bool))
    v = base.copy()
    v[[5, 40, 63]] = 3.0                                                # ties: the smallest lane wins
    wave(v, np.ones(64, bool))
    wave(np.full(64, 0.25), np.ones(64, bool))                          # all equal: lane 0
    wave(base, np.zeros(64, bool))                                      # no lane has one
    has = np.zeros(64, bool)
    has[[9, 33]] = True
    wave(np.full(64, 7.0), has)                                         # two holders among idle lanes
    has = rng.random(64) < 0.3
    has[60] = True
    wave(rng.random(64) ** 6, has)
    v = np.concatenate([w[0] for w in waves])
    h = np.concatenate([w[1] for w in waves])
    pad = (-len(v)) % 256
    v, h = np.concatenate([v, np.full(pad, -np.inf)]), np.concatenate([h, np.zeros(pad, bool)])
    rec = np.zeros((len(v), 2), u8)
    rec[:, 0], rec[:, 1] = bits(v), h
    r = run(OP["PT_WAVE_FIRST_MAX"], rec, u8, 2 * len(v)).reshape(-1, 2)
    for k in range(len(v) // 64):
        vv, hh = v[64 * k:64 * k + 64], h[64 * k:64 * k + 64]
        m = vv[hh].max() if hh.any() else -np.inf
        lane = int(np.nonzero(hh & (vv == m))[0][0]) if hh.any() else 0
        assert np.all(r[64 * k:64 * k + 64, 0] == bits([m])[0]) and np.all(r[64 * k:64 * k + 64, 1].view(i8) == lane), \
            "wave %d: (%r, %d), expected (%r, %d)" % (k, r[64 * k, 0:1].view(f8)[0], r[64 * k, 1], m, lane)


# ==== 3 x 3 algebra ===================================================================================================
def matrices3():
    """symmetric positive definite 3 x 3 (full storage, bitwise symmetric): well conditioned and of condition 1e12; and general
    ones (S = H P H^T + R is not bitwise symmetric): the same with the last bits of the lower triangle moved"""
    rng = np.random.default_rng(0x3A3A)
    n = 2050
    V = _rotations(rng, n)
    lam = 10.0 ** rng.uniform(-3, 1, (n, 3))
    lam[n // 2:] = 10.0 ** rng.uniform(-2, 2, (n - n // 2, 1)) * np.array([1.0, 1e-6, 1e-12])
    S = np.einsum("nij,nj,nkj->nik", V, lam, V)
    S = 0.5 * (S + np.transpose(S, (0, 2, 1)))
    G = S.copy()
    G[:, TRI[1], TRI[0]] = G[:, TRI[0], TRI[1]] * (1 + rng.integers(-4, 5, (n, 6)) * ULP)
    d = rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-3, 3, (n, 1))
    return S[:, TRI[0], TRI[1]].copy(), G.reshape(n, 9).copy(), d


def numpy_inv_sym3(P):
    xx, xy, xz, yy, yz, zz = P.T
    c00 = yy * zz - yz * yz
    c01 = xy * zz - yz * xz
    c02 = xy * yz - yy * xz
    det = xx * c00 - xy * c01 + xz * c02
    i = 1.0 / det
    return np.stack([c00 * i, (xz * yz - xy * zz) * i, (xy * yz - xz * yy) * i, (xx * zz - xz * xz) * i, (xz * xy - xx * yz) * i,
                     (xx * yy - xy * xy) * i, det], 1)


def numpy_inv_gen3(a):
    a = a.T
    c00 = a[4] * a[8] - a[5] * a[7]
    c01 = a[3] * a[8] - a[5] * a[6]
    c02 = a[3] * a[7] - a[4] * a[6]
    det = a[0] * c00 - a[1] * c01 + a[2] * c02
    i = 1.0 / det
    return np.stack([c00 * i, (a[2] * a[7] - a[1] * a[8]) * i, (a[1] * a[5] - a[2] * a[4]) * i, (a[5] * a[6] - a[3] * a[8]) * i,
                     (a[0] * a[8] - a[2] * a[6]) * i, (a[2] * a[3] - a[0] * a[5]) * i, c02 * i, (a[1] * a[6] - a[0] * a[7]) * i,
                     (a[0] * a[4] - a[1] * a[3]) * i, det], 1)


def numpy_quad(A, d, sym):
    A, (d0, d1, d2) = A.T, d.T
    ix = (0, 1, 2, 1, 3, 4, 2, 4, 5) if sym else range(9)
    r = [A[ix[3 * t]] * d0 + A[ix[3 * t + 1]] * d1 + A[ix[3 * t + 2]] * d2 for t in range(3)]
    return d0 * r[0] + d1 * r[1] + d2 * r[2]


def check_algebra3(run):
    """bit-equal to unfused arithmetic in the order of the source (numpy does not fuse): what PHD_REF_ARITH is for"""
    S, G, d = matrices3()
    n = len(S)
    assert np.array_equal(bits(run(OP["PT_INV_SYM3"], S, f8, 7 * n).reshape(n, 7)), bits(numpy_inv_sym3(S))), "inv_sym3"
    assert np.array_equal(bits(run(OP["PT_INV_GEN3"], G, f8, 10 * n).reshape(n, 10)), bits(numpy_inv_gen3(G))), "inv_gen3"
    assert np.array_equal(bits(run(OP["PT_QUAD_SYM"], np.concatenate([S, d], 1), f8, n)), bits(numpy_quad(S, d, True))), "quad_sym"
    assert np.array_equal(bits(run(OP["PT_QUAD_GEN"], np.concatenate([G, d], 1), f8, n)), bits(numpy_quad(G, d, False))), "quad_gen"
