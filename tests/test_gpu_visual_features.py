"""gcs_visual_features on the MI355X: the device rows against tests/visual_features_ref.py's restatement of
the node on every fixture (the criteria of tests/test_visual_features_host.py: visual_features_ref.check),
bitwise repeatability, and the chain depth image -> features -> camera slice -> live scan without a host
copy: the device features through CameraSplatBuilder.build and, in a CameraFrame, through
process_scan_single_hypothesis, bit for bit what the same arrays give when downloaded and passed as a host
dict; and the raw C call on a side stream, read by a dependent torch op with no synchronise in between."""

import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import visual_features_ref as VR
from gcslam import _lib as L
from gcslam import visual as V
from gcslam.camera import CameraFrame, CameraSplatBuilder, DepthFusionConfig, PinholeIntrinsics

pytestmark = pytest.mark.gpu

FEATURES = [n for n, _, _ in L.VISFEAT_FEATURE_FIELDS]
DIAG = [n for n, _, _ in L.VISFEAT_DIAG_FIELDS]


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def device_rows(case):
    """A case through gcs_visual_features, all max_features rows, downloaded."""
    out = V.extract_visual_features(case["depth"], case["rgb"], case["keypoints"], PinholeIntrinsics(*case["intrinsics"]),
                                    config=V.VisualFeatureConfig(**case["cfg"]), want_diag=True, trim=False)
    return _np(out), _np(out.diag), out.count


@pytest.mark.parametrize("name", VR.CASE_NAMES)
def test_device_meets_the_criteria(name):
    case = VR.BY_NAME[name]
    got, diag, count = device_rows(case)
    fig = VR.check(got, diag, count, case, "device")
    print(f"{name}: {count} rows, {fig['n_fit']} fitted, largest residual / bound {fig['residual']:.3f}")


@pytest.mark.parametrize("name", ["holes_median5", "holes_hex", "noisy_fit_r3", "select_1100", "uint16"])
def test_two_calls_are_byte_identical(name):
    a, b = device_rows(VR.BY_NAME[name]), device_rows(VR.BY_NAME[name])
    for x, y in ((a[0], b[0]), (a[1], b[1])):
        for k in x:
            assert x[k].tobytes() == y[k].tobytes(), k


def test_device_tensors_with_a_row_pitch():
    """torch tensors in, a depth image that is a view of a wider one: the packed image's rows."""
    case = VR.BY_NAME["holes_median3"]
    K, cfg = PinholeIntrinsics(*case["intrinsics"]), V.VisualFeatureConfig(**case["cfg"])
    want = V.extract_visual_features(case["depth"], case["rgb"], case["keypoints"], K, config=cfg, want_diag=True)
    wide = torch.full((VR.H, VR.W + 8), 3.0, dtype=torch.float32, device="cuda")
    wide[:, :VR.W] = torch.from_numpy(case["depth"]).cuda()
    kp = torch.from_numpy(case["keypoints"]).cuda()
    got = V.extract_visual_features(wide[:, :VR.W], torch.from_numpy(case["rgb"]).cuda(), (kp[:, 0], kp[:, 1], kp[:, 2]),
                                    K, config=cfg, want_diag=True)
    assert got.count == want.count == len(case["keypoints"]) and got["cov"].shape == (got.count, 9)
    for k in FEATURES:
        assert got[k].cpu().numpy().tobytes() == want[k].cpu().numpy().tobytes(), k


# ---- chaining: a 640 x 480 frame seen by tests/test_gpu_live_camera.py's camera

def _frame_inputs(m=96, seed=3):
    import test_gpu_live_camera as LC
    g = np.random.default_rng(seed)
    y, x = np.mgrid[0:480, 0:640].astype(np.float64)
    depth = (3.0 + 0.002 * (x - 320.0) - 0.001 * (y - 240.0) + 0.01 * g.standard_normal((480, 640))).astype(np.float32)
    depth[g.integers(0, 480, 400), g.integers(0, 640, 400)] = np.nan
    rgb = g.integers(0, 256, (480, 640, 3), dtype=np.uint8)
    kp = np.stack([g.uniform(20, 620, m), g.uniform(20, 460, m), g.uniform(1.0, 200.0, m)], 1).astype(np.float32)
    return LC, depth, rgb, kp


@pytest.fixture(scope="module")
def frame_features():
    LC, depth, rgb, kp = _frame_inputs()
    dev = V.extract_visual_features(depth, rgb, kp, LC.K)
    assert getattr(dev, "_on_device", False) and dev.count == 96 and dev["u"].is_cuda
    host = {k: v.cpu().numpy() for k, v in dev.items()}
    assert host["has_mu"].sum() > 80 and (host["weight"] > 0).sum() > 80
    return LC, dev, host


def test_device_features_go_straight_into_build(frame_features):
    LC, dev, host = frame_features
    g = np.random.default_rng(4)
    pix = np.stack([g.uniform(0, 640, 2000), g.uniform(0, 480, 2000)], 1)
    z = 3.0 + 0.05 * g.standard_normal(2000)
    pc = np.stack([(pix[:, 0] - LC.K.cx) / LC.K.fx * z, (pix[:, 1] - LC.K.cy) / LC.K.fy * z, z], 1)
    cloud = pc @ LC.R_BC.T + LC.T_BC
    b = CameraSplatBuilder(DepthFusionConfig(lidar_projection_radius_pix=8.0), max_points=8192)
    one = b.build(dev, cloud, LC.K, LC.R_BC, LC.T_BC, 100.05, want_diag=True)
    two = b.build(host, cloud, LC.K, LC.R_BC, LC.T_BC, 100.05, want_diag=True)
    assert one.n_camera_valid == two.n_camera_valid == 96
    for f in LC.BATCH:
        LC._same(f"batch.{f}", getattr(one, f), getattr(two, f))
    for k in one.camera_diag:
        LC._same(f"camera_diag.{k}", one.camera_diag[k], two.camera_diag[k])
    assert one.camera_diag["fused"].sum().item() > 0   # the LiDAR depth fusion ran on these features
    b.close()


@pytest.mark.parametrize("chain", [True, False])
def test_device_frame_through_the_live_scan(frame_features, chain, monkeypatch):
    """One scan with a primitive map and camera_batch_policy="use": the frame once of device features, once of
    the downloaded arrays -- the batch, visual_pose, the belief and everything else _same_result compares."""
    LC, dev, host = frame_features
    monkeypatch.setenv("GCSLAM_LIVE_CHAIN", "1" if chain else "0")
    seen = LC._spy(monkeypatch)
    frames = (CameraFrame(dev, LC.K, LC.R_BC, LC.T_BC, 100.05, config=LC.FUSION, want_diag=True),
              CameraFrame(host, LC.K, LC.R_BC, LC.T_BC, 100.05, config=LC.FUSION, want_diag=True))
    assert frames[0].arrays is None and frames[0].device_arrays is dev and frames[0].n_features == 96
    assert frames[1].device_arrays is None
    res = []
    for fr in frames:
        p = LC.Pair(LC._config())
        res.append(p.scan(0, fr))
        p.close()
    assert len(seen) == (2 if chain else 0)
    LC._same_result("device vs host frame", res[0], res[1])
    assert res[0].measurement_batch.n_camera_valid == 96


def test_camera_frame_validates_device_features(frame_features):
    LC, dev, host = frame_features
    bad = type(dev)(dev)
    bad["xyz"] = dev["xyz"][:, :2]
    with pytest.raises(ValueError, match="xyz"):
        CameraFrame(bad, LC.K, LC.R_BC, LC.T_BC, 1.0)
    bad = type(dev)(dev)
    bad["weight"] = dev["weight"].to(torch.float32)
    with pytest.raises(ValueError, match="weight"):
        CameraFrame(bad, LC.K, LC.R_BC, LC.T_BC, 1.0)
    big = type(dev)((k, torch.zeros((65536,) + tuple(v.shape[1:]), dtype=v.dtype, device="cuda")) for k, v in dev.items())
    with pytest.raises(ValueError, match="65535"):
        CameraFrame(big, LC.K, LC.R_BC, LC.T_BC, 1.0)


def test_camera_frame_from_rgbd(frame_features):
    LC, dev, host = frame_features
    _, depth, rgb, kp = _frame_inputs()
    f = V.camera_frame_from_rgbd(depth, rgb, kp, LC.K, LC.R_BC, LC.T_BC, 100.05, fusion_config=LC.FUSION)
    assert f.arrays is None and f.n_features == 96 and f.config == LC.FUSION
    for k in FEATURES:
        assert f.device_arrays[k].cpu().numpy().tobytes() == host[k].tobytes(), k


def test_raw_call_on_a_side_stream_orders_a_dependent_op(lib):
    """The C entry through raw pointers on a torch stream other than the default; a torch op queued after it on
    that stream, with no synchronise in between, reads the finished arrays."""
    case = VR.BY_NAME["noisy_fit_r2"]
    want, _, count = device_rows(case)
    cfg = V.VisualFeatureConfig(**case["cfg"])
    c = V.config_struct(cfg)
    h = C.c_void_p()
    assert lib.gcs_visfeat_ctx_create(C.byref(c), C.byref(h)) == 0
    side = torch.cuda.Stream()
    depth, rgb = torch.from_numpy(case["depth"]).cuda(), torch.from_numpy(case["rgb"]).cuda()
    kp = [torch.from_numpy(np.ascontiguousarray(case["keypoints"][:, j])).cuda() for j in range(3)]
    rows = cfg.max_features
    arrs = {n: torch.full((rows, w) if w else (rows,), 77, dtype=getattr(torch, dt), device="cuda")
            for n, w, dt in L.VISFEAT_FEATURE_FIELDS}
    torch.cuda.synchronize()   # the inputs above were made on the default stream
    i = V._inputs_struct(depth.data_ptr(), 0, depth.stride(0) * 4, VR.W, VR.H, rgb.data_ptr(), rgb.stride(0),
                         PinholeIntrinsics(*case["intrinsics"]), len(kp[0]), [k.data_ptr() for k in kp])
    o = L.GcsVisfeatOutputs()
    for n, x in arrs.items():
        setattr(o, n, x.data_ptr())
    assert lib.gcs_visfeat_ctx_set_stream(h, C.c_void_p(side.cuda_stream)) == 0
    with torch.cuda.stream(side):
        assert lib.gcs_visual_features(h, C.byref(i), C.byref(o)) == 0, lib.gcs_visfeat_last_error(h)
        total = arrs["xyz"].sum(dim=0) + arrs["weight"].sum()   # queued behind the kernels on the same stream
        copy = {n: x.clone() for n, x in arrs.items()}
    assert o.count == count
    side.synchronize()
    for n in FEATURES:
        assert copy[n].cpu().numpy().tobytes() == want[n].tobytes(), n
    # (two sums of under 50 non-zero terms in another order: 50 * 2^-53 of the terms' magnitudes at the most)
    np.testing.assert_allclose(total.cpu().numpy(), want["xyz"].sum(0) + want["weight"].sum(), rtol=0,
                               atol=1e-14 * (np.abs(want["xyz"]).sum() + want["weight"].sum()))
    assert lib.gcs_visfeat_ctx_destroy(h) == 0
