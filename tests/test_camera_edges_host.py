"""CPU checks of the camera-splat edge fixtures (tests/golden/camera_edges_*.npz, recorded from the
reference by tests/golden/make_camera_splats_edges.py): the conditions on the reference's inputs that
tests/test_gpu_camera_splats_edges.py relies on, so that a later regeneration cannot quietly hollow
those tests out, and the padding helper's clouds against the recorded digests."""

import os

import numpy as np
import pytest

from camera_pad import PADDED_SIZES, digest, filler, pad_cloud, stored_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CASES = ("r8_A", "r8_B", "r3_A", "fit_A", "depth_A", "r8_E")
CLASSES = ((0, 0), (1, 2), (3, 64), (65, 256), (257, 1024), (1025, 1 << 30))


def _load(name):
    return dict(np.load(os.path.join(GOLD, f"camera_edges_{name}.npz")))


@pytest.fixture(scope="module")
def scene():
    return _load("scene")


@pytest.fixture(scope="module")
def cases():
    return {c: _load(c) for c in CASES}


def _cfg(scene, cid):
    row = scene["cfg_values"][list(scene["config_ids"]).index(cid)]
    return dict(zip((str(x) for x in scene["cfg_names"]), row))


def test_files_are_small_and_complete(scene, cases):
    for name in ("scene",) + CASES:
        assert os.path.getsize(os.path.join(GOLD, f"camera_edges_{name}.npz")) < 200 * 1024, name
    assert [str(x) for x in scene["cases"]] == list(CASES)
    m = scene["u"].shape[0]
    assert 257 <= m <= 512 and scene["points"].dtype == np.float32
    for name, c in cases.items():
        for k in ("n_pt", "z_med", "mad", "Lambda_A", "theta_A", "Lambda_B", "theta_B", "fused", "z_f", "weights",
                  "plane_determined", "z_raw", "sig_raw", "ndotr"):
            assert c[k].shape == (m,), (name, k)
        assert c["Lambdas"].shape == (m, 3, 3) and c["thetas"].shape == c["eta0"].shape == c["colors"].shape == (m, 3)
        if name != "r8_B":
            assert np.array_equal(c["R_base_camera"], np.eye(3)) and not c["t_base_camera"].any()
    R = cases["r8_B"]["R_base_camera"]
    np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-14)
    assert cases["r8_B"]["points_base"].dtype == np.float32 and cases["r8_B"]["points_base"].shape == scene["points"].shape


def test_configs_are_the_recorded_ones(scene):
    from gcslam.camera import DepthFusionConfig
    names = [str(x) for x in scene["cfg_names"]]
    d = DepthFusionConfig()
    assert [getattr(d, k) for k in names] == list(scene["cfg_defaults"])
    assert _cfg(scene, "r3") == dict(zip(names, scene["cfg_defaults"]))      # the reference's default config
    assert _cfg(scene, "r8")["lidar_projection_radius_pix"] == 8.0
    fit, dep = _cfg(scene, "fit"), _cfg(scene, "depth")
    assert (fit["lidar_ray_plane_fit_max_points"], fit["lidar_plane_fit_min_points"], fit["gamma_lidar"],
            fit["depth_fusion_weight_camera"], fit["depth_fusion_weight_lidar"]) == (16, 5, 0.5, 0.7, 1.3)
    assert (dep["depth_min_m"], dep["depth_sigma_max_sq"]) == (30.0, 1e-3)
    for cid in ("r8", "fit", "depth"):      # each differs from the default only where stated
        diff = {k for k in names if _cfg(scene, cid)[k] != _cfg(scene, "r3")[k]}
        assert diff == {"r8": {"lidar_projection_radius_pix"},
                        "fit": {"lidar_projection_radius_pix", "lidar_ray_plane_fit_max_points",
                                "lidar_plane_fit_min_points", "gamma_lidar", "depth_fusion_weight_camera",
                                "depth_fusion_weight_lidar"},
                        "depth": {"lidar_projection_radius_pix", "depth_min_m", "depth_sigma_max_sq"}}[cid]


def test_scene_and_features_hold_the_edge_cases(scene):
    p = scene["points"].astype(np.float64)
    nan_rows = np.isnan(p).all(axis=1)
    assert nan_rows.sum() >= 3 and not (np.isnan(p).any(axis=1) & ~nan_rows).any()      # all-NaN rows only
    z = p[~nan_rows, 2]
    assert (z < 0).sum() >= 32 and z.max() > 45.0 and 0 < z[z > 0].min() < 2.6
    assert (z == 3.0).sum() >= 1000                                  # the exact z = const patch
    u, v = scene["u"], scene["v"]
    fx, fy, cx, cy = scene["intrinsics"]
    assert u[0] == cx and v[0] == cy                                 # the principal point itself
    assert (u < 0).sum() >= 3 and (u > 640).sum() >= 3               # outside the image on both sides
    m = u.shape[0]
    assert (scene["depth_Lambda_c"] == 0).sum() == (m + 4) // 5 and (~scene["has_mu"]).sum() == (m + 1) // 3
    assert (~scene["has_color"]).sum() == (m + 1) // 4
    assert (scene["color"] < 0).any() and (scene["color"] > 1).any()


def test_undetermined_share_and_class_coverage(scene, cases):
    for name in CASES[:-1]:
        c = cases[name]
        runs_b = np.isfinite(c["z_raw"])
        min_pts = _cfg(scene, name.split("_")[0])["lidar_plane_fit_min_points"]
        assert np.array_equal(runs_b, c["n_pt"] >= min_pts), name
        assert np.array_equal(np.isfinite(c["z_med"]), runs_b), name
        und = (runs_b & ~c["plane_determined"]).sum()
        assert und <= 0.20 * runs_b.sum(), (name, und, runs_b.sum())
        assert c["plane_determined"][~runs_b].all()
        assert 0 < (~c["fused"]).sum() < c["fused"].shape[0]
    for name in ("r8_A", "r8_B"):
        n, det = cases[name]["n_pt"], cases[name]["plane_determined"]
        counts = [int(((n >= lo) & (n <= hi) & det).sum()) for lo, hi in CLASSES]
        assert all(x >= 3 for x in counts), (name, counts)
    n = cases["r8_A"]["n_pt"]
    assert n[n <= 1024].max() > 900                                   # near the LDS cap of 1,024
    fit = cases["fit_A"]
    assert ((fit["n_pt"] > 16) & fit["plane_determined"]).sum() >= 3   # idle lanes in the plane-fit wave
    assert ((fit["n_pt"] >= 3) & (fit["n_pt"] < 5)).sum() >= 1         # min_points = 5 excludes what 3 admits
    assert not fit["Lambda_A"][fit["n_pt"] < 5].any()
    assert cases["r3_A"]["n_pt"].max() <= 1024                         # every feature runs at radius 3


def test_equal_depths_and_scalar_branches(scene, cases):
    a = cases["r8_A"]
    tie = a["mad"] == 0.0
    assert tie.sum() >= 3 and (tie & (a["n_pt"] > 256)).any() and (tie & (a["n_pt"] <= 256)).any()
    assert (a["z_med"][tie] == 3.0).all()
    det = a["plane_determined"]
    x = a["z_raw"] - _cfg(scene, "r8")["depth_min_m"]
    assert (det & (x > 20.0)).any() and (det & (x > 0.0) & (x <= 20.0)).any()         # softplus: x > 20 and the log arm
    t_angle = _cfg(scene, "r8")["plane_angle_sigmoid_t"]
    assert (det & (np.abs(a["ndotr"]) < 0.05)).any() and (det & (np.abs(a["ndotr"]) > t_angle)).any()   # grazing floor
    d = cases["depth_A"]
    det, cf = d["plane_determined"], _cfg(scene, "depth")
    x = d["z_raw"] - cf["depth_min_m"]
    assert (det & (x < -20.0)).any()                                   # softplus: x < -20
    assert (det & (x < 0.0) & (x >= -20.0)).any()                      # w_behind with the log arm
    assert (det & (x > 0.0)).any()
    assert (det & (d["sig_raw"] > cf["depth_sigma_max_sq"])).any()     # the sigma_max_sq clamp
    assert (det & (d["sig_raw"] < cf["depth_sigma_max_sq"])).any()
    assert (d["Lambda_B"][det & (x < -20.0)] > 0).all()                # tiny, not zero: the branch reaches the output


def test_no_lidar_case_keeps_or_backprojects_the_input(scene, cases):
    e = cases["r8_E"]
    assert not e["n_pt"].any() and not e["Lambda_A"].any() and not e["Lambda_B"].any()
    assert np.array_equal(e["fused"], scene["depth_Lambda_c"] > 0)
    keep = ~e["fused"]
    Lam = np.linalg.inv(scene["cov_in"][keep] + float(scene["eps_lift"]) * np.eye(3))
    np.testing.assert_allclose(e["Lambdas"][keep], Lam, rtol=1e-9, atol=0)
    np.testing.assert_allclose(e["z_f"][~keep], (scene["depth_theta_c"] / np.maximum(scene["depth_Lambda_c"], 1e-300))[~keep],
                               rtol=1e-15)


def test_padding_helper_reproduces_the_digests(scene):
    assert tuple(int(x) for x in scene["padded_sizes"]) == PADDED_SIZES == (16500, 65536, 66000)
    pts = scene["points"]
    n = pts.shape[0]
    for n_total, want in zip(PADDED_SIZES, scene["padded_sha256"]):
        cloud = pad_cloud(pts, n_total)
        assert cloud.shape == (n_total, 3) and cloud.dtype == np.float32
        assert digest(cloud) == str(want), n_total
        rows = stored_rows(n, n_total)
        assert np.array_equal(cloud[rows], pts, equal_nan=True)         # stored points in order
        blocks = np.unique(rows // 256)
        nblk = -(-n_total // 256)
        assert np.array_equal(blocks, np.arange(nblk))                  # in every block of the scan
        fill = np.ones(n_total, bool)
        fill[rows] = False
        f = cloud[fill].astype(np.float64)
        assert np.array_equal(f, filler(n_total - n).astype(np.float64))
        behind = f[:, 2] < 0
        assert abs(int(behind.sum()) - int((~behind).sum())) <= 1       # half behind, half in front
        fx, _, cx, _ = scene["intrinsics"]
        assert (fx * f[~behind, 0] / f[~behind, 2] + cx > scene["u"].max() + 1000.0).all()   # far outside every box
        assert np.array_equal(f * 16.0, np.round(f * 16.0))             # dyadic: exact in float32
    assert -(-PADDED_SIZES[0] // 256) == 65 and PADDED_SIZES[1] == 256 * 256 and -(-PADDED_SIZES[2] // 256) == 258
