"""gcs_camera_splats_scan (the camera slice from the scan's own records) against gcs_camera_splats on the
float64 array of the same values, on tests/golden/camera_splats.npz (case B: a real camera extrinsic; its
points are stored as float32, so every record form holds the same values).  Widening float32 is exact, so
every batch array and every diagnostic must be equal bit for bit.

Record forms: float32 x, y, z with point_step 12 and 16 (xyz_format 0) and float64 with step 24
(xyz_format 1).  Point counts 0, 1, 255, 257 and the fixture's own: one short of and one past a 256-thread
block of k_cs_count / k_cs_compact (two blocks, so k_cs_offsets' prefix carries from block 0 to block 1).
The points within a feature's radius come first in the order used, so the short counts are all kept points
and every count past 0 gives candidates."""

import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from gcslam import _lib as L
from gcslam.camera import CameraSplatBuilder, DepthFusionConfig, PinholeIntrinsics

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = (0, 1, 255, 257, None)   # None: the fixture's own
FORMS = ((12, 0), (16, 0), (24, 1))


@pytest.fixture(scope="module")
def setup():
    fx = dict(np.load(os.path.join(ROOT, "tests", "golden", "camera_splats.npz")))
    feats = dict(u=fx["u"], v=fx["v"], depth_Lambda_c=fx["depth_Lambda_c"], depth_theta_c=fx["depth_theta_c"],
                 xyz=fx["xyz_in"], cov=fx["cov_in"], weight=fx["weight"], kappa_app=fx["kappa_app"],
                 mu_app=fx["mu_app"], has_mu=fx["has_mu"], color=fx["color"], has_color=fx["has_color"])
    p32 = fx["B_points_base"]
    assert p32.dtype == np.float32 and p32.shape[0] > 257
    R, t = fx["B_R_base_camera"], fx["B_t_base_camera"]
    K = PinholeIntrinsics(*fx["intrinsics"])
    # the points within the radius of some feature first (stable), so a short prefix is all candidates
    pc = (p32.astype(np.float64) - t) @ R
    z = pc[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v = K.fx * pc[:, 0] / z + K.cx, K.fy * pc[:, 1] / z + K.cy
    d2 = (u[:, None] - fx["u"][None]) ** 2 + (v[:, None] - fx["v"][None]) ** 2
    near = (z > 0) & (np.nan_to_num(d2, nan=np.inf).min(axis=1) <= float(fx["radius"]) ** 2)
    assert near.sum() > 257
    p32 = np.ascontiguousarray(p32[np.argsort(~near, kind="stable")])
    b = CameraSplatBuilder(DepthFusionConfig(lidar_projection_radius_pix=float(fx["radius"])), n_feat=128,
                           n_surfel=64, eps_lift=float(fx["eps_lift"]), max_points=max(8192, p32.shape[0]))
    fa = b.device_features(feats)
    args = (K, R, t, float(fx["timestamp"]))
    yield dict(b=b, fa=fa, p32=p32, args=args, ref={})
    b.close()


def _host(batch):
    out = {k: getattr(batch, k).cpu().numpy() for k in L.CAMSPLAT_BATCH_FIELDS}
    out.update({"diag_" + k: v.cpu().numpy() for k, v in batch.camera_diag.items()})
    out["n_camera_valid"] = np.int64(batch.n_camera_valid)
    return out


def _reference(s, n):
    """gcs_camera_splats on the float64 array of the first n points: once per count, shared."""
    if n not in s["ref"]:
        p = torch.as_tensor(s["p32"][:n].astype(np.float64), device=DEV)
        s["ref"][n] = _host(s["b"].build(s["fa"], p, *s["args"], want_diag=True))
    return s["ref"][n]


@pytest.mark.parametrize("step,fmt", FORMS)
@pytest.mark.parametrize("count", COUNTS)
def test_records_equal_the_float64_array_bit_for_bit(setup, count, step, fmt):
    s = setup
    n = s["p32"].shape[0] if count is None else count
    ref = _reference(s, n)
    p = s["p32"][:n]
    if fmt == 0:
        rec = np.full((max(n, 1), step // 4), 7.5, np.float32)   # the record's padding is never read as a coordinate
        rec[:n, :3] = p
    else:
        rec = np.zeros((max(n, 1), 3), np.float64)
        rec[:n] = p
    got = _host(s["b"].build_from_records(s["fa"], torch.as_tensor(rec, device=DEV), step, fmt, n, *s["args"],
                                          want_diag=True))
    n_pt = ref["diag_n_pt"]
    print(f"n={n} step={step} fmt={fmt}: features with candidates {(n_pt > 0).sum()}, candidates {n_pt.sum()}")
    assert ref["n_camera_valid"] == 96
    if n > 0:
        assert n_pt.sum() > 0          # the comparison sees fused features
    if n >= 257:
        assert n_pt.sum() >= 257       # kept points in both blocks
    assert set(got) == set(ref)
    for k in ref:
        assert got[k].dtype == ref[k].dtype and got[k].tobytes() == ref[k].tobytes(), k


def test_bad_record_forms_are_refused(setup):
    s = setup
    rec = torch.zeros((4, 4), dtype=torch.float32, device=DEV)
    for step, fmt in ((8, 0), (14, 0), (16, 1), (28, 1), (12, 2)):
        with pytest.raises(ValueError):
            s["b"].build_from_records(s["fa"], rec, step, fmt, 2, *s["args"])
    with pytest.raises(ValueError):   # more records asked for than the tensor holds
        s["b"].build_from_records(s["fa"], rec, 16, 0, 5, *s["args"])
