"""CPU checks of the camera rows of the one-call live scan: the library exports gcs_live_scan_camera and
gcs_camera_splats_scan beside what existed, the ABI version and the layout of every struct bound before
them are unchanged, null arguments are refused without a device, and gcslam.camera.CameraFrame validates
what it is given."""

import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gcs_live_scan_camera", "gcs_camera_splats_scan")
# sizeof of every struct _lib.py bound before the camera rows (ABI 4)
SIZES = {"GcsAssocConfig": 112, "GcsAssocMeas": 56, "GcsAssocOutputs": 224, "GcsAssocView": 72, "GcsBelief": 4280,
         "GcsCamsplatConfig": 224, "GcsCamsplatInputs": 256, "GcsCamsplatOutputs": 152, "GcsConfig": 160,
         "GcsImuOdomInputs": 176, "GcsLidarEvidence": 48, "GcsLiveArgs": 352, "GcsLiveOutputs": 2512,
         "GcsPmapRows": 88, "GcsPmapUpdateConfig": 80, "GcsPmapUpdateInputs": 104, "GcsPmapUpdateStats": 48,
         "GcsPmapView": 96, "GcsPointCloud2Layout": 144, "GcsRenderConfig": 96, "GcsRenderPrepareInputs": 104,
         "GcsRenderSplats": 48, "GcsScanBeginOutputs": 656, "GcsScanInputs": 192, "GcsScanOutputs": 16024,
         "GcsSurfelConfig": 112, "GcsSurfelOutputs": 176, "GcsVpeOutputs": 4280}


def test_new_entry_points_declared_and_exported(lib):
    from gcslam import _lib as L
    hdr = open(os.path.join(ROOT, "include", "gcslam_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int64_t|const char\*)\s+(gcs_\w+)\s*\(", hdr, re.M))
    for name in NEW_SYMBOLS:
        assert name in declared and name in L.SYMBOLS and hasattr(lib, name), name
    assert "gcs_live_camera;" in hdr
    assert lib.gcs_abi_version() == 4 and L.ABI_VERSION == 4


def test_existing_struct_layouts_are_unchanged():
    from gcslam import _lib as L
    for name, size in SIZES.items():
        assert C.sizeof(getattr(L, name)) == size, name
    # the new struct: three pointers, three int32 (+ pad), a pointer, an int32 (+ pad), a pointer
    assert C.sizeof(L.GcsLiveCamera) == 64
    assert [f[0] for f in L.GcsLiveCamera._fields_] == ["ctx", "inputs", "xyz_dev", "point_step", "xyz_format",
                                                         "n_points", "src", "n_feat", "out"]


def test_null_arguments_are_refused(lib):
    from gcslam import _lib as L
    ERR_ARG = -1
    i, o = L.GcsCamsplatInputs(), L.GcsCamsplatOutputs()
    assert lib.gcs_camera_splats_scan(None, C.byref(i), None, 12, 0, 0, C.byref(o)) == ERR_ARG
    assert lib.gcs_camera_splats(None, C.byref(i), C.byref(o)) == ERR_ARG
    bo, a, lo, out = L.GcsScanBeginOutputs(), L.GcsLiveArgs(), L.GcsLiveOutputs(), L.GcsScanOutputs()
    cam = L.GcsLiveCamera()
    assert lib.gcs_live_scan_camera(None, None, C.byref(bo), C.byref(a), C.byref(cam), C.byref(lo),
                                    C.byref(out)) == ERR_ARG
    assert lib.gcs_live_scan_camera(None, None, None, None, None, None, None) == ERR_ARG
    assert lib.gcs_live_scan(None, None, None, None, None, None) == ERR_ARG


def _features(m=4):
    return dict(u=np.arange(m, dtype=float), v=np.ones(m), xyz=np.ones((m, 3)), cov=np.tile(np.eye(3), (m, 1, 1)),
                weight=np.ones(m), kappa_app=np.ones(m))


def test_camera_frame_validation():
    from gcslam.camera import CameraFrame, DepthFusionConfig, PinholeIntrinsics
    K = PinholeIntrinsics(400.0, 410.0, 320.0, 240.0)
    f = CameraFrame(_features(), K, np.eye(3), [0.1, 0.0, 0.2], 12.5)
    assert f.n_features == f.n_valid == 4 and f.config == DepthFusionConfig() and not f.want_diag
    assert f.arrays["cov"].shape == (4, 9) and f.arrays["has_mu"].tolist() == [0] * 4
    assert f.R_base_camera.shape == (3, 3) and f.t_base_camera.shape == (3,) and f.max_candidates == 1024
    assert CameraFrame(_features(0), K, np.eye(3), np.zeros(3), 0.0).n_valid == 0   # an empty frame: no camera batch
    with pytest.raises(ValueError):
        CameraFrame(_features(), K, np.eye(4), np.zeros(3), 0.0)
    with pytest.raises(ValueError):
        CameraFrame(_features(), K, np.eye(3), np.zeros(2), 0.0)
    with pytest.raises(ValueError):
        CameraFrame(_features(), K, np.full((3, 3), np.nan), np.zeros(3), 0.0)
    with pytest.raises(ValueError):
        CameraFrame(_features(), PinholeIntrinsics(0.0, 1.0, 0.0, 0.0), np.eye(3), np.zeros(3), 0.0)
    with pytest.raises(ValueError):
        CameraFrame(_features(), K, np.eye(3), np.zeros(3), float("inf"))
    with pytest.raises(ValueError):
        CameraFrame(_features(), K, np.eye(3), np.zeros(3), 0.0, max_candidates=1025)
    with pytest.raises(TypeError):
        CameraFrame(_features(), K, np.eye(3), np.zeros(3), 0.0, config=dict(lidar_projection_radius_pix=3.0))
    bad = _features()
    del bad["weight"]
    with pytest.raises(KeyError):
        CameraFrame(bad, K, np.eye(3), np.zeros(3), 0.0)
    bad = _features()
    bad["xyz"] = np.ones((4, 2))
    with pytest.raises(ValueError):
        CameraFrame(bad, K, np.eye(3), np.zeros(3), 0.0)


def test_the_pipeline_counts_a_frame_as_a_camera_batch():
    from gcslam import pipeline
    from gcslam.camera import CameraFrame, PinholeIntrinsics
    K = PinholeIntrinsics(400.0, 400.0, 320.0, 240.0)
    assert pipeline._camera_batch_has_content(CameraFrame(_features(3), K, np.eye(3), np.zeros(3), 0.0))
    assert not pipeline._camera_batch_has_content(CameraFrame(_features(0), K, np.eye(3), np.zeros(3), 0.0))
