"""gcs_detect_keypoints_pyramid on the MI355X: the device result against tests/keypoints_pyramid_ref.py's numpy
restatement of the definition on every fixture, rgb and gray, compared as bytes (the comparisons of
tests/test_keypoints_pyramid_host.py); one level against KeypointDetector; bitwise repeatability; a context reused
for smaller images, whose level offsets move; row pitch; the trimmed result; the chain into the feature operator
from Python and through the raw C route with n_keypoints = max_keypoints and the NaN padding."""

import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import keypoints_pyramid_ref as PR
import keypoints_ref as KR
import test_keypoints_pyramid_host as TH
from gcslam import _lib as L
from gcslam import keypoints as KP
from gcslam import visual as V
from gcslam.camera import PinholeIntrinsics

pytestmark = pytest.mark.gpu

FEATURES = [n for n, _, _ in L.VISFEAT_FEATURE_FIELDS]
RS = 1e-3   # response_soft_scale: the detector's responses are 1e-4 .. 1e-2, so w_resp = r / (r + RS) is not ~0


def all_rows(det, image):
    """Every max_keypoints row of one call, downloaded, with .level, .counts and .level_counts."""
    rows, level, words = det.queue(image)
    torch.cuda.synchronize()
    return KP._pyramid_result([r.cpu().numpy() for r in rows], level.cpu().numpy(), words.cpu().tolist())


def device(name, image=None, **over):
    cfg = KP.PyramidConfig(**PR.config(name, **over))
    img = PR.image(name) if image is None else image
    return all_rows(KP._pyramid_detector_for(cfg, 0, img.shape[0], img.shape[1]), np.array(img))


@pytest.mark.parametrize("name", PR.NAMES)
def test_device_equals_the_restatement(name):
    ref = PR.expected(name)
    K = PR.config(name)["max_keypoints"]
    got = device(name)
    print(f"{name}: counts {got.counts} level_counts {got.level_counts}")
    TH.same_as_ref(got, ref, K, name)
    if PR.image(name).ndim == 3:   # the fixture is rgb: its own grey image gives the same bytes
        TH.same_as_ref(device(name, KR.grey(PR.image(name))), ref, K, (name, "gray"))
    else:                          # the fixture is gray: the same value in three channels is that grey again
        TH.same_as_ref(device(name, np.repeat(np.array(PR.image(name))[:, :, None], 3, 2)), ref, K, (name, "rgb"))


@pytest.mark.parametrize("name", PR.NAMES)
def test_detect_returns_trimmed_device_tensors(name):
    ref = PR.expected(name)
    got = KP.detect_keypoints_pyramid(np.array(PR.image(name)), KP.PyramidConfig(**PR.config(name)))
    n = ref["counts"][0]
    assert got.counts == ref["counts"] and np.array(got.level_counts, np.int32).tobytes() == ref["level_counts"].tobytes()
    assert len(got) == 3 and all(t.is_cuda and t.shape == (n,) and t.dtype == torch.float32 for t in got)
    assert got.level.is_cuda and got.level.shape == (n,) and got.level.dtype == torch.int32
    for t, k in zip(tuple(got) + (got.level,), TH.ROWS + ("level",)):
        assert t.cpu().numpy().tobytes() == ref[k].tobytes(), (name, k)


@pytest.mark.parametrize("name", KR.NAMES)
def test_one_level_is_the_keypoint_detector(name):
    cfg = KR.config(name)
    img = np.array(KR.image(name))
    one = KP.KeypointDetector(KP.KeypointConfig(**cfg))
    rows, counts = one.queue(img)
    pyr = KP.PyramidDetector(KP.PyramidConfig(n_levels=1, **cfg))
    got = all_rows(pyr, img)
    want = counts.cpu().tolist()
    assert list(got.counts[:3]) == want[:3] == list(KR.expected(name)["counts"]) and got.counts[3] == 1
    for a, b in zip(rows, got):
        assert a.cpu().numpy().tobytes() == b.tobytes()
    n = want[0]
    assert (got.level[:n] == 0).all() and (got.level[n:] == -1).all()
    one.close()
    pyr.close()


def test_two_calls_are_byte_identical():
    for name in ("vga_k4096", "vga_k512", "dots_64x96_l3_k16"):
        a, b = device(name), device(name)
        assert a.counts[0] == PR.config(name)["max_keypoints"]
        TH.same_bytes(a, b)


def test_a_reused_context_keeps_nothing_of_a_larger_frame():
    """vga, then 61 x 97, then 9 x 9 on one context: every level's offset in the packed workspace moves."""
    cfg = KP.PyramidConfig(**PR.config("blocks_61x97_l3", max_width=640, max_height=480))
    names = ("vga", "blocks_61x97", "dot_9x9")
    one = KP.PyramidDetector(cfg)
    reused = [all_rows(one, np.array(KR.image(n))) for n in names]
    one.close()
    for n, got in zip(names, reused):
        fresh = KP.PyramidDetector(cfg)
        TH.same_bytes(got, all_rows(fresh, np.array(KR.image(n))))
        fresh.close()
    TH.same_as_ref(reused[1], PR.expected("blocks_61x97_l3"), 4096, "blocks_61x97 after vga")
    assert reused[0].counts[0] > 1000 and reused[2].counts[:2] == (1, 1)


@pytest.mark.parametrize("name", ["blocks_61x97_l3", "wide_130x35_l3", "noise_48x64_l3", "dots_64x96_l3", "blocks_60x96_l3_s2"])
def test_a_torch_view_keeps_its_row_pitch(name):
    img = torch.from_numpy(np.array(PR.image(name))).cuda()
    H, W = img.shape[0], img.shape[1]
    wide = torch.full((H, W + 7) + tuple(img.shape[2:]), 255, dtype=torch.uint8, device="cuda")
    wide[:, :W] = img
    view = wide[:, :W]
    assert not view.is_contiguous()
    det = KP.PyramidDetector(KP.PyramidConfig(**PR.config(name)))
    assert det._image(view)[0].data_ptr() == wide.data_ptr()   # passed as it is, rows (W + 7) pixels apart
    got = all_rows(det, view)
    TH.same_bytes(got, all_rows(det, img))
    TH.same_as_ref(got, PR.expected(name), 4096, name)
    det.close()


def test_device_entry_refuses_bad_inputs(lib):
    det = KP.PyramidDetector(KP.PyramidConfig(max_width=64, max_height=64, max_keypoints=64))
    buf = torch.zeros(4 * 64 + 36, dtype=torch.float32, device="cuda")
    img = torch.zeros((64, 192), dtype=torch.uint8, device="cuda")
    ptrs = [buf[j * 64:].data_ptr() for j in range(4)] + [buf[256:].data_ptr(), buf[260:].data_ptr()]
    for field, value in TH.BAD_INPUTS:
        i = KP._inputs_struct(img.data_ptr(), 1, 192, 32, 32)
        o = L.GcsKeypointPyramidOutputs(*ptrs)
        setattr(i if hasattr(i, field) else o, field, {33: 65}.get(value, value))
        assert lib.gcs_detect_keypoints_pyramid(det.h, C.byref(i), C.byref(o)) == -1, (field, value)
        assert lib.gcs_keypoint_pyramid_last_error(det.h)
    with pytest.raises(ValueError):
        det.detect(torch.zeros((65, 8), dtype=torch.uint8))
    det.close()


# ---- chaining

@pytest.fixture(scope="module")
def frame():
    import test_gpu_visual_features as TV
    LC, depth, _, _ = TV._frame_inputs()
    return LC, depth, np.array(KR.image("vga"))


def test_extract_runs_the_pyramid_for_a_pyramid_config(frame):
    LC, depth, rgb = frame
    cfg = V.VisualFeatureConfig(response_soft_scale=RS)
    pc = KP.PyramidConfig(max_keypoints=512)
    kp = KP.detect_keypoints_pyramid(rgb, pc)
    ref = PR.expected("vga_k512")
    assert kp.counts == ref["counts"] and kp[0].cpu().numpy().tobytes() == ref["u"].tobytes()
    a = V.extract_visual_features(depth, rgb, None, LC.K, config=cfg, keypoint_config=pc)
    b = V.extract_visual_features(depth, rgb, kp, LC.K, config=cfg)   # the pyramid's result is a valid keypoints argument
    c = V.extract_visual_features(depth, rgb, tuple(k.cpu().numpy() for k in kp), LC.K, config=cfg)
    assert a.count == b.count == c.count == 512
    for k in FEATURES:
        assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes() == c[k].cpu().numpy().tobytes(), k
    # every keypoint is a feature here, written in input order: u, v are the level-0 sub-pixel coordinates widened
    order = a["kp_index"].cpu().numpy() if "kp_index" in a else np.arange(512)
    assert a["u"].cpu().numpy().tobytes() == ref["u"][order].astype(np.float64).tobytes()
    assert a["v"].cpu().numpy().tobytes() == ref["v"][order].astype(np.float64).tobytes()
    assert (ref["u"] != np.round(ref["u"])).any()
    # another detector than the level-0 one ran
    d = V.extract_visual_features(depth, rgb, None, LC.K, config=cfg, keypoint_config=KP.KeypointConfig(max_keypoints=512))
    assert d["u"].cpu().numpy().tobytes() != a["u"].cpu().numpy().tobytes()
    f = V.camera_frame_from_rgbd(depth, rgb, None, LC.K, LC.R_BC, LC.T_BC, 100.05, config=cfg, fusion_config=LC.FUSION,
                                 keypoint_config=pc)
    assert f.arrays is None and f.n_features == 512
    for k in FEATURES:
        assert f.device_arrays[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k


def test_c_route_chains_with_the_nan_padding_and_no_wait(lib):
    """gcs_detect_keypoints_pyramid, then gcs_visual_features with n_keypoints = max_keypoints and the NaN-padded
    arrays, both queued on a side stream with nothing between them: the real keypoints' rows are those of the
    trimmed route, every further row weighs 0."""
    name, cap = "blocks_61x97_l3", 512
    rgb = np.array(PR.image(name))
    H, W = rgb.shape[:2]
    n = PR.expected(name)["counts"][0]
    assert 0 < n < cap
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    depth = (2.0 + 0.004 * x - 0.002 * y).astype(np.float32)
    K = PinholeIntrinsics(80.0, 80.0, W / 2.0, H / 2.0)
    # (the quotas of cap = 512 still hold every level's survivors: 147, 100, 67)
    pcfg = KP.PyramidConfig(**PR.config(name, max_keypoints=cap, max_width=128, max_height=128))
    vcfg = V.VisualFeatureConfig(max_features=cap, max_keypoints=cap, response_soft_scale=RS)
    trimmed = KP.detect_keypoints_pyramid(rgb, pcfg)
    assert trimmed.counts[0] == n
    want = V.extract_visual_features(depth, rgb, trimmed, K, config=vcfg, trim=False)
    assert want.count == n
    want = {k: v.cpu().numpy() for k, v in want.items()}

    pc, vc = KP.pyramid_config_struct(pcfg), V.config_struct(vcfg)
    ph, vh = C.c_void_p(), C.c_void_p()
    assert lib.gcs_keypoint_pyramid_ctx_create(C.byref(pc), C.byref(ph)) == 0
    assert lib.gcs_visfeat_ctx_create(C.byref(vc), C.byref(vh)) == 0
    side = torch.cuda.Stream()
    rgb_d, depth_d = torch.from_numpy(rgb).cuda(), torch.from_numpy(depth).cuda()
    kp = torch.full((3, cap), 7.0, dtype=torch.float32, device="cuda")
    level = torch.full((cap,), 99, dtype=torch.int32, device="cuda")
    words = torch.full((36,), -1, dtype=torch.int32, device="cuda")
    arrs = {k: torch.full((cap, w) if w else (cap,), 77, dtype=getattr(torch, dt), device="cuda")
            for k, w, dt in L.VISFEAT_FEATURE_FIELDS}
    torch.cuda.synchronize()   # the inputs above were made on the default stream
    ki = KP._inputs_struct(rgb_d.data_ptr(), 3, rgb_d.stride(0), W, H)
    ko = L.GcsKeypointPyramidOutputs(kp[0].data_ptr(), kp[1].data_ptr(), kp[2].data_ptr(), level.data_ptr(),
                                     words.data_ptr(), words[4:].data_ptr())
    vi = V._inputs_struct(depth_d.data_ptr(), 0, depth_d.stride(0) * 4, W, H, rgb_d.data_ptr(), rgb_d.stride(0), K, cap,
                          [kp[j].data_ptr() for j in range(3)])
    vo = L.GcsVisfeatOutputs()
    for k, a in arrs.items():
        setattr(vo, k, a.data_ptr())
    assert lib.gcs_keypoint_pyramid_ctx_set_stream(ph, C.c_void_p(side.cuda_stream)) == 0
    assert lib.gcs_visfeat_ctx_set_stream(vh, C.c_void_p(side.cuda_stream)) == 0
    assert lib.gcs_detect_keypoints_pyramid(ph, C.byref(ki), C.byref(ko)) == 0, lib.gcs_keypoint_pyramid_last_error(ph)
    assert lib.gcs_visual_features(vh, C.byref(vi), C.byref(vo)) == 0, lib.gcs_visfeat_last_error(vh)
    side.synchronize()
    ref = PR.expected(name)
    assert words.cpu().tolist()[:4] == [n, n, ref["counts"][2], 3] and vo.count == cap
    assert level.cpu().numpy()[:n].tobytes() == ref["level"].tobytes() and (level.cpu().numpy()[n:] == -1).all()
    got = {k: a.cpu().numpy() for k, a in arrs.items()}
    for k in FEATURES:
        assert got[k][:n].tobytes() == want[k][:n].tobytes(), k
    assert (got["weight"][n:] == 0).all() and (got["weight"][:n] > 0).any()
    assert lib.gcs_keypoint_pyramid_ctx_destroy(ph) == 0 and lib.gcs_visfeat_ctx_destroy(vh) == 0
