"""Large clouds for the camera-splat edge tests, built from a small stored cloud (pure numpy, no RNG).

pad_cloud(points, n_total) spreads the stored points evenly over n_total rows (stored point i lands in
row i * n_total // n, so they fall in every 256-point block of the scan) and fills the other rows with
points that no feature can see: even filler rows lie behind the camera, odd ones in front of it but at
pixels far outside the image (u >= 3,520 with the fixtures' pinhole), so the count of points in front of
the camera and the count the compaction keeps differ.  Filler coordinates are small dyadic rationals
from integer arithmetic, exact in float32; the stored points keep their order, so every candidate set
holds the same points in the same order as in the stored cloud."""

import hashlib

import numpy as np

PADDED_SIZES = (16500, 65536, 66000)   # 65 blocks (two waves of the scan), max_points, 258 blocks (two per thread)


def filler(n):
    """(n, 3) float32: row j behind the camera for even j, in front and far to the right for odd j."""
    j = np.arange(n, dtype=np.int64)
    out = np.empty((n, 3), np.float32)
    even = j % 2 == 0
    zb = -(1.0 + (j % 128) / 16.0)                  # -1 .. -8.94 m
    zf = 1.0 + (j % 64) / 16.0                      # 1 .. 4.94 m
    out[:, 0] = np.where(even, ((j * 7) % 64 - 32) / 8.0, 8.0 * zf)      # x / z = 8: u = fx * 8 + cx
    out[:, 1] = np.where(even, ((j * 5) % 32 - 16) / 8.0, ((j * 3) % 16) / 8.0)
    out[:, 2] = np.where(even, zb, zf)
    return out


def stored_rows(n, n_total):
    """Rows of the padded cloud that hold the stored points, increasing."""
    return (np.arange(n, dtype=np.int64) * n_total) // n


def pad_cloud(points, n_total):
    points = np.ascontiguousarray(points, np.float32)
    n = points.shape[0]
    assert points.shape == (n, 3) and n_total >= n > 0
    rows = stored_rows(n, n_total)
    is_stored = np.zeros(n_total, bool)
    is_stored[rows] = True
    assert int(is_stored.sum()) == n
    out = np.empty((n_total, 3), np.float32)
    out[rows] = points
    out[~is_stored] = filler(n_total - n)
    return out


def digest(cloud):
    return hashlib.sha256(np.ascontiguousarray(cloud, np.float32).tobytes()).hexdigest()
