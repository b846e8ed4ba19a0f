"""gcs_detect_keypoints on the MI355X: the device result against tests/keypoints_ref.py's numpy restatement of
the definition on every fixture, compared as bytes (the comparisons of tests/test_keypoints_host.py); bitwise
repeatability; a context reused for smaller images; row pitch; the chain image -> keypoints -> features ->
CameraFrame without a host copy; and the raw C route, detector and feature operator queued back to back on a
side stream with n_keypoints = max_keypoints and the NaN padding."""

import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import keypoints_ref as KR
import test_keypoints_host as TH
from gcslam import _lib as L
from gcslam import keypoints as KP
from gcslam import visual as V
from gcslam.camera import PinholeIntrinsics

pytestmark = pytest.mark.gpu

FEATURES = [n for n, _, _ in L.VISFEAT_FEATURE_FIELDS]


def all_rows(det, image):
    """Every max_keypoints row of one call, downloaded, with .counts."""
    rows, counts = det.queue(image)
    torch.cuda.synchronize()
    out = KP.Keypoints(r.cpu().numpy() for r in rows)
    out.counts = tuple(int(v) for v in counts.cpu().tolist())
    return out


def device(name, **over):
    cfg = KP.KeypointConfig(**KR.config(name, **over))
    img = KR.image(name)
    return all_rows(KP._detector_for(cfg, 0, img.shape[0], img.shape[1]), np.array(img))


def same_bytes(a, b):
    assert a.counts == b.counts
    for x, y in zip(a, b):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()


@pytest.mark.parametrize("name", KR.NAMES)
def test_device_equals_the_restatement(name):
    ref = KR.expected(name)
    got = device(name)
    TH.same_as_ref(got, ref, 4096, name)
    trimmed = KP.detect_keypoints(np.array(KR.image(name)), KP.KeypointConfig(**KR.config(name)))
    assert trimmed.counts == got.counts and all(t.is_cuda and t.shape == (got.counts[0],) for t in trimmed)
    for t, g in zip(trimmed, got):
        assert t.cpu().numpy().tobytes() == g[:got.counts[0]].tobytes()
    print(f"{name}: counts {got.counts}")


@pytest.mark.parametrize("name,cap", TH.CAPS + (("vga", 512),))
def test_caps_keep_the_top_n_in_raster_order(name, cap):
    ref = KR.expected(name, max_keypoints=cap)
    got = device(name, max_keypoints=cap)
    TH.same_as_ref(got, ref, cap, (name, cap))
    assert got.counts[0] == cap and got.counts[1] == KR.expected(name)["counts"][1] > cap
    TH.check_cap([a[:cap] for a in got], name, cap)


def test_two_calls_are_byte_identical():
    a, b = device("vga"), device("vga")
    assert a.counts[0] > 512
    same_bytes(a, b)
    same_bytes(device("vga", max_keypoints=512), device("vga", max_keypoints=512))


def test_a_reused_context_keeps_nothing_of_a_larger_frame():
    cfg = KP.KeypointConfig(**KR.config("blocks_61x97", max_width=128, max_height=128))
    names = ("blocks_61x97", "blocks_48x64", "dot_9x9")
    one = KP.KeypointDetector(cfg)
    reused = [all_rows(one, np.array(KR.image(n))) for n in names]
    one.close()
    for n, got in zip(names, reused):
        fresh = KP.KeypointDetector(cfg)
        same_bytes(got, all_rows(fresh, np.array(KR.image(n))))
        fresh.close()
        TH.same_as_ref(got, KR.expected(n), 4096, n)


@pytest.mark.parametrize("name", ["blocks_61x97", "wide_130x35", "noise_48x64", "dots_64x96"])
def test_a_torch_view_keeps_its_row_pitch(name):
    img = torch.from_numpy(np.array(KR.image(name))).cuda()
    H, W = img.shape[0], img.shape[1]
    wide = torch.full((H, W + 8) + tuple(img.shape[2:]), 255, dtype=torch.uint8, device="cuda")
    wide[:, :W] = img
    view = wide[:, :W]
    assert not view.is_contiguous()
    det = KP.KeypointDetector(KP.KeypointConfig(**KR.config(name)))
    assert det._image(view)[0].data_ptr() == wide.data_ptr()   # passed as it is, rows (W + 8) pixels apart
    got = all_rows(det, view)
    same_bytes(got, all_rows(det, img))
    TH.same_as_ref(got, KR.expected(name), 4096, name)
    det.close()


def test_device_entry_refuses_bad_inputs(lib):
    det = KP.KeypointDetector(KP.KeypointConfig(max_width=64, max_height=64, max_keypoints=64))
    buf = torch.zeros(4 * 64, dtype=torch.float32, device="cuda")
    img = torch.zeros((64, 192), dtype=torch.uint8, device="cuda")
    o = L.GcsKeypointOutputs(*(buf[j * 64:].data_ptr() for j in range(4)))
    for field, value in TH.BAD_INPUTS:
        i = KP._inputs_struct(img.data_ptr(), 1, 192, 32, 32)
        oo = L.GcsKeypointOutputs(o.kp_u, o.kp_v, o.kp_response, o.counts)
        setattr(i if hasattr(i, field) else oo, field, {33: 65}.get(value, value))
        assert lib.gcs_detect_keypoints(det.h, C.byref(i), C.byref(oo)) == -1, (field, value)
        assert lib.gcs_keypoint_last_error(det.h)
    with pytest.raises(ValueError):
        det.detect(torch.zeros((65, 8), dtype=torch.uint8))
    det.close()


# ---- chaining

RS = 1e-3   # response_soft_scale: the detector's responses are 1e-4 .. 1e-2, so w_resp = r / (r + RS) is not ~0


@pytest.fixture(scope="module")
def frame():
    import test_gpu_visual_features as TV
    LC, depth, _, _ = TV._frame_inputs()
    return LC, depth, np.array(KR.image("vga"))


def test_extract_detects_when_no_keypoints_are_given(frame):
    LC, depth, rgb = frame
    cfg = V.VisualFeatureConfig(response_soft_scale=RS)
    kp = KP.detect_keypoints(rgb)
    assert kp.counts[0] == KR.expected("vga")["counts"][0] > 512
    kp_host = tuple(k.cpu().numpy() for k in kp)
    a = V.extract_visual_features(depth, rgb, None, LC.K, config=cfg)
    b = V.extract_visual_features(depth, rgb, kp_host, LC.K, config=cfg)
    c = V.extract_visual_features(depth, rgb, kp, LC.K, config=cfg)   # detect's tuple is a valid keypoints argument
    assert a.count == b.count == c.count == 512
    for k in FEATURES:
        assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes() == c[k].cpu().numpy().tobytes(), k
    assert (a["weight"] > 0).sum().item() > 256
    f = V.camera_frame_from_rgbd(depth, rgb, None, LC.K, LC.R_BC, LC.T_BC, 100.05, config=cfg, fusion_config=LC.FUSION)
    assert f.arrays is None and f.n_features == 512
    for k in FEATURES:
        assert f.device_arrays[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k
    with pytest.raises(ValueError, match="rgb"):
        V.extract_visual_features(depth, None, None, LC.K, config=cfg)


def test_keypoint_config_reaches_the_detector(frame):
    LC, depth, rgb = frame
    cfg = V.VisualFeatureConfig(response_soft_scale=RS)
    kc = KP.KeypointConfig(max_keypoints=100, fast_threshold=30)
    a = V.extract_visual_features(depth, rgb, None, LC.K, config=cfg, keypoint_config=kc)
    b = V.extract_visual_features(depth, rgb, KP.detect_keypoints(rgb, kc), LC.K, config=cfg)
    assert a.count == b.count == 100
    for k in FEATURES:
        assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k


def test_c_route_chains_with_the_nan_padding_and_no_wait(lib):
    """gcs_detect_keypoints, then gcs_visual_features with n_keypoints = max_keypoints and the NaN-padded arrays,
    both queued on a side stream with nothing between them: the real keypoints' rows are those of the trimmed
    route, every further row weighs 0."""
    name, cap = "blocks_61x97", 256
    rgb = np.array(KR.image(name))
    H, W = rgb.shape[:2]
    n = KR.expected(name)["counts"][0]
    assert 0 < n < cap
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    depth = (2.0 + 0.004 * x - 0.002 * y).astype(np.float32)
    K = PinholeIntrinsics(80.0, 80.0, W / 2.0, H / 2.0)
    kcfg = KP.KeypointConfig(**KR.config(name, max_keypoints=cap, max_width=128, max_height=128))
    vcfg = V.VisualFeatureConfig(max_features=cap, max_keypoints=cap, response_soft_scale=RS)
    want = V.extract_visual_features(depth, rgb, KP.detect_keypoints(rgb, kcfg), K, config=vcfg, trim=False)
    assert want.count == n
    want = {k: v.cpu().numpy() for k, v in want.items()}

    kc, vc = KP.config_struct(kcfg), V.config_struct(vcfg)
    kh, vh = C.c_void_p(), C.c_void_p()
    assert lib.gcs_keypoint_ctx_create(C.byref(kc), C.byref(kh)) == 0
    assert lib.gcs_visfeat_ctx_create(C.byref(vc), C.byref(vh)) == 0
    side = torch.cuda.Stream()
    rgb_d, depth_d = torch.from_numpy(rgb).cuda(), torch.from_numpy(depth).cuda()
    kp = torch.full((3, cap), 7.0, dtype=torch.float32, device="cuda")
    counts = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    arrs = {k: torch.full((cap, w) if w else (cap,), 77, dtype=getattr(torch, dt), device="cuda")
            for k, w, dt in L.VISFEAT_FEATURE_FIELDS}
    torch.cuda.synchronize()   # the inputs above were made on the default stream
    ki = KP._inputs_struct(rgb_d.data_ptr(), 3, rgb_d.stride(0), W, H)
    ko = L.GcsKeypointOutputs(kp[0].data_ptr(), kp[1].data_ptr(), kp[2].data_ptr(), counts.data_ptr())
    vi = V._inputs_struct(depth_d.data_ptr(), 0, depth_d.stride(0) * 4, W, H, rgb_d.data_ptr(), rgb_d.stride(0), K, cap,
                          [kp[j].data_ptr() for j in range(3)])
    vo = L.GcsVisfeatOutputs()
    for k, a in arrs.items():
        setattr(vo, k, a.data_ptr())
    assert lib.gcs_keypoint_ctx_set_stream(kh, C.c_void_p(side.cuda_stream)) == 0
    assert lib.gcs_visfeat_ctx_set_stream(vh, C.c_void_p(side.cuda_stream)) == 0
    assert lib.gcs_detect_keypoints(kh, C.byref(ki), C.byref(ko)) == 0, lib.gcs_keypoint_last_error(kh)
    assert lib.gcs_visual_features(vh, C.byref(vi), C.byref(vo)) == 0, lib.gcs_visfeat_last_error(vh)
    side.synchronize()
    assert counts.cpu().tolist() == [n, n, KR.expected(name)["counts"][2], 0] and vo.count == cap
    got = {k: a.cpu().numpy() for k, a in arrs.items()}
    for k in FEATURES:
        assert got[k][:n].tobytes() == want[k][:n].tobytes(), k
    assert (got["weight"][n:] == 0).all() and (got["weight"][:n] > 0).any()
    assert lib.gcs_keypoint_ctx_destroy(kh) == 0 and lib.gcs_visfeat_ctx_destroy(vh) == 0
