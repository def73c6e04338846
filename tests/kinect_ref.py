"""A second reading, in numpy, of the Kinect model's detection probability: KinectMeasurer.FuzzyVisibleM
(KinectMeasurer.cs:151-173) times detectionProbability (SimulatedVehicle.cs:335-338), on top of the PRM3D FuzzyVisibleM
(PRM3DMeasurer.cs:277-291). np.float32 arithmetic where the C# uses float: the pixel offset ResX / 2, the range cast and
the two subtractions; double elsewhere. The depth map is row-major depth[y][x] (include/phdhip.h, phd_set_depth_map).

Written from the reference's source, independently of the device code (phd_device.h)."""
import numpy as np


def prm3d_visible(p, z):
    """PRM3DMeasurer.FuzzyVisibleM clamped to [0, 1], vectorised over z[n][3]: the smallest of the six border distances
    over their ramps (integer film rectangle, float32 range clip)."""
    z = np.asarray(z, np.float64).reshape(-1, 3)
    left, top = int(p.measurer[3]), int(p.measurer[4])
    right, bottom = left + int(p.measurer[5]), top + int(p.measurer[6])
    rmin, rmax = float(np.float32(p.measurer[1])), float(np.float32(p.measurer[2]))
    ramp = [float(r) for r in p.visibility_ramp]
    d = np.minimum.reduce([(z[:, 0] - left) / ramp[0], (right - z[:, 0]) / ramp[0],
                           (z[:, 1] - top) / ramp[1], (bottom - z[:, 1]) / ramp[1],
                           (z[:, 2] - rmin) / ramp[2], (rmax - z[:, 2]) / ramp[2]])
    return np.maximum(0.0, np.minimum(1.0, d))


def pixel(depth, z):
    """(x, y, inside): x = (int) (X + ResX / 2), y = (int) (Y + ResY / 2) with ResX / 2 a float32 division; `inside` is
    False where that pixel is not in the image (the library then gives PD 0; the reference would throw)."""
    z = np.asarray(z, np.float64).reshape(-1, 3)
    h, w = np.asarray(depth).shape
    xd = z[:, 0] + float(np.float32(w) / np.float32(2))
    yd = z[:, 1] + float(np.float32(h) / np.float32(2))
    inside = (xd > -1.0) & (xd < w) & (yd > -1.0) & (yd < h)
    x = np.where(inside, np.trunc(np.where(inside, xd, 0.0)), 0).astype(np.int64)
    y = np.where(inside, np.trunc(np.where(inside, yd, 0.0)), 0).astype(np.int64)
    return x, y, inside


def detection_probability(p, z, depth=None):
    """DetectionProbabilityM at pixel-range points z[n][3]; depth None: the PRM3D value."""
    z = np.asarray(z, np.float64).reshape(-1, 3)
    base = prm3d_visible(p, z)
    if depth is None:
        return base * p.pd
    depth = np.asarray(depth, np.float32)
    x, y, inside = pixel(depth, z)
    d = np.where(inside, depth[y, x], np.float32(-np.inf)).astype(np.float32)
    r = z[:, 2].astype(np.float32)
    ramp2 = float(p.visibility_ramp[2])
    with np.errstate(invalid="ignore", over="ignore"):
        t_range = (r - np.float32(p.measurer[1])).astype(np.float64) / ramp2   # float32 subtraction, double division
        t_depth = (d - r).astype(np.float64) / ramp2
        m = np.minimum(np.minimum(base, t_range), t_depth)
    v = np.maximum(0.0, np.minimum(1.0, m))
    v = np.where((base == 0) | np.isnan(d), 0.0, v)
    return v * p.pd


def occluding_map(rng, width, height, near=0.5, far=1.5, blocks=(8, 6), holes=0.05):
    """piecewise-constant occluders: a blocks[0] x blocks[1] grid of depths uniform in [near, far], and a fraction of
    NaN holes (no reading)"""
    bx, by = blocks
    cell = rng.uniform(near, far, (by, bx)).astype(np.float32)
    ys = np.minimum(np.arange(height) * by // height, by - 1)
    xs = np.minimum(np.arange(width) * bx // width, bx - 1)
    d = cell[ys[:, None], xs[None, :]].copy()
    d[rng.uniform(size=d.shape) < holes] = np.nan
    return d


def probe_points(rng, w, h, n):
    """n pixel-range points over a w x h image and 12 pixels beyond each side, ranges in [0, 4.2]; a quarter of them on a
    pixel edge exactly or one ulp either side of it"""
    hx, hy = w / 2, h / 2
    z = np.column_stack([rng.uniform(-hx - 12, hx + 12, n), rng.uniform(-hy - 12, hy + 12, n), rng.uniform(0.0, 4.2, n)])
    k = n // 4   # pixel edges: exactly on a cell boundary and one ulp either side
    ex = rng.integers(-int(hx) - 2, int(hx) + 2, k).astype(float)
    ey = rng.integers(-int(hy) - 2, int(hy) + 2, k).astype(float)
    side = rng.integers(0, 3, (k, 2))
    ex = np.where(side[:, 0] == 0, np.nextafter(ex, -np.inf), np.where(side[:, 0] == 1, ex, np.nextafter(ex, np.inf)))
    ey = np.where(side[:, 1] == 0, np.nextafter(ey, -np.inf), np.where(side[:, 1] == 1, ey, np.nextafter(ey, np.inf)))
    z[:k, 0], z[:k, 1] = ex, ey
    return z


def probe_map(rng, w, h):
    """a w x h map of depths in [0, 4.5] with NaN, +inf, -inf, 0 and below-RangeClip.Min pixels among them"""
    d = rng.uniform(0.0, 4.5, (h, w)).astype(np.float32)
    kind = rng.integers(0, 8, (h, w))
    d[kind == 0] = np.nan
    d[kind == 1] = np.inf
    d[kind == 2] = -np.inf
    d[kind == 3] = 0.0
    d[kind == 4] = np.float32(0.05)   # below RangeClip.Min
    return d
