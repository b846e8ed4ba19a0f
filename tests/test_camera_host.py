"""CPU checks of the camera-splat operator's host side: the fixture recorded from the reference
(tests/golden/camera_splats.npz, written by tests/golden/make_camera_splats.py) carries the cases the
GPU tests rely on, the Python config mirrors the reference's recorded defaults, the C-ABI declares and
exports the new entry points, and the pipeline accepts the "use" policy."""

import ctypes as C
import dataclasses
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "camera_splats.npz")
NEW_SYMBOLS = ("gcs_camsplat_config_defaults", "gcs_camsplat_ctx_create", "gcs_camsplat_ctx_destroy",
               "gcs_camsplat_last_error", "gcs_camsplat_ctx_set_stream", "gcs_camera_splats")


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(FIXTURE))


def test_fixture_is_small_and_covers_the_candidate_classes(fx):
    assert os.path.getsize(FIXTURE) < 200 * 1024
    m = fx["u"].shape[0]
    assert m == 96 and float(fx["radius"]) == 8.0
    min_pts = int(fx["cfg_values"][list(fx["cfg_names"]).index("lidar_plane_fit_min_points")])
    for case in "AB":
        n = fx[f"{case}_n_pt"]
        assert n.shape == (m,) and fx[f"{case}_points_base"].dtype == np.float32
        classes = [(n == 0).sum(), ((n >= 1) & (n <= 2)).sum(), ((n >= 3) & (n <= 64)).sum(), (n > 64).sum()]
        assert all(c > 0 for c in classes), classes
        assert (n > 32).sum() > 0                      # the capacity test's dense-patch features
        fused = fx[f"{case}_fused"]
        assert 0 < (~fused).sum() < m                  # keep-the-input and fused features both present
        assert np.array_equal(np.isfinite(fx[f"{case}_z_med"]), n >= min_pts)
        # a kept input is the incoming splat, moved to the base frame
        R, t = fx[f"{case}_R_base_camera"], fx[f"{case}_t_base_camera"]
        keep = ~fused
        assert np.array_equal(fx[f"{case}_cam_xyz"][keep], fx["xyz_in"][keep])
        np.testing.assert_allclose(fx[f"{case}_base_xyz"][keep], fx["xyz_in"][keep] @ R.T + t, rtol=1e-13, atol=1e-13)
    assert np.array_equal(fx["A_R_base_camera"], np.eye(3)) and not fx["A_t_base_camera"].any()
    R = fx["B_R_base_camera"]
    np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-14)
    # the feature mix: one in five without camera depth, one in three without mu_app, one in four without colour
    assert (fx["depth_Lambda_c"] == 0).sum() == 20 and (~fx["has_mu"]).sum() == 32 and (~fx["has_color"]).sum() == 24
    assert (fx["color"] < 0).any() and (fx["color"] > 1).any()   # the clip is exercised


def test_config_defaults_equal_the_references(fx):
    from gcslam import _lib as L
    from gcslam.camera import DepthFusionConfig
    names = [str(x) for x in fx["cfg_names"]]
    cfg = DepthFusionConfig()
    assert [f.name for f in dataclasses.fields(cfg)] == names
    c = L.GcsCamsplatConfig()
    assert L.load().gcs_camsplat_config_defaults(C.byref(c)) == 0
    for name, val, is_int in zip(names, fx["cfg_values"], fx["cfg_is_int"]):
        assert getattr(cfg, name) == val and isinstance(getattr(cfg, name), int) == bool(is_int), name
        assert getattr(c, name) == val, name
    assert (c.pixel_sigma, c.eps_lift, c.n_feat, c.n_surfel, c.max_candidates) == (1.0, 1e-9, 512, 1024, 1024)


def test_new_symbols_declared_and_exported(lib):
    from gcslam import _lib as L
    hdr = open(os.path.join(ROOT, "include", "gcslam_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int64_t|const char\*)\s+(gcs_\w+)\s*\(", hdr, re.M))
    for name in NEW_SYMBOLS:
        assert name in declared and name in L.SYMBOLS and hasattr(lib, name), name
    assert lib.gcs_abi_version() == 4
    assert lib.gcs_camsplat_last_error(None) == b"null camera-splat context"


def test_invalid_config_is_refused_without_a_device(lib):
    from gcslam import _lib as L
    c = L.GcsCamsplatConfig()
    lib.gcs_camsplat_config_defaults(C.byref(c))
    h = C.c_void_p()
    for field, bad in (("max_candidates", 1025), ("max_candidates", 0), ("lidar_ray_plane_fit_max_points", 65),
                       ("n_feat", 0), ("max_points", 0)):
        c2 = L.GcsCamsplatConfig.from_buffer_copy(c)
        setattr(c2, field, bad)
        assert lib.gcs_camsplat_ctx_create(C.byref(c2), C.byref(h)) == -1 and not h.value, field


def test_pipeline_accepts_the_use_policy():
    from gcslam import pipeline
    assert pipeline.CAMERA_BATCH_POLICIES == ("warn", "raise", "ignore", "use")
    assert pipeline.PipelineConfig().camera_batch_policy == "warn"
    assert pipeline.PipelineConfig(camera_batch_policy="use").camera_batch_policy == "use"
    with pytest.raises(ValueError):
        pipeline.PipelineConfig(camera_batch_policy="fuse")


def test_feature_arrays_from_objects_and_dicts(fx):
    from gcslam.camera import feature_arrays

    @dataclasses.dataclass
    class F:   # Feature3D's attribute names
        u: float
        v: float
        xyz: np.ndarray
        cov_xyz: np.ndarray
        weight: float
        meta: dict
        mu_app: object = None
        kappa_app: float = 0.0
        color: object = None

    feats = [F(1.0, 2.0, np.arange(3.0), np.eye(3), 0.5, {"depth_Lambda_c": 4.0, "depth_theta_c": 8.0},
               np.array([0.0, 0.0, 1.0]), 3.0, np.array([0.1, 0.2, 0.3])),
             F(3.0, 4.0, np.ones(3), 2 * np.eye(3), 0.25, {})]
    a = feature_arrays(feats)
    assert a["u"].tolist() == [1.0, 3.0] and a["depth_Lambda_c"].tolist() == [4.0, 0.0]
    assert a["depth_theta_c"].tolist() == [8.0, 0.0] and a["has_mu"].tolist() == [1, 0]
    assert a["has_color"].tolist() == [1, 0] and a["cov"].shape == (2, 9) and a["cov"][1, 4] == 2.0
    d = feature_arrays(dict(u=a["u"], v=a["v"], xyz=a["xyz"], cov=a["cov"].reshape(2, 3, 3), weight=a["weight"],
                            kappa_app=a["kappa_app"]))
    assert d["has_mu"].tolist() == [0, 0] and d["depth_Lambda_c"].tolist() == [0.0, 0.0] and d["cov"].shape == (2, 9)
    assert feature_arrays([])["u"].shape == (0,)
