"""gcs_detect_keypoints_grid on the MI355X: the device result against tests/keypoints_grid_ref.py's numpy restatement
of G1-G4 on every fixture, rgb and gray, compared as bytes (the comparisons of tests/test_keypoints_grid_host.py);
what the definition reduces to against PyramidDetector and KeypointDetector; bitwise repeatability; a context
reused for smaller images; row pitch; the chain into the feature operator from Python and through the raw C route
with n_keypoints = max_keypoints and the NaN padding.  The shapes are the smallest at which the new kernels can go
wrong: a partial last cell (96 x 64 at cell 16), a cap of 0 with a remainder, a cap >= 2 with a remainder, levels
without cells behind levels with cells, all-equal keys; ramp_vga_k512 is the only large frame."""

import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import keypoints_grid_ref as GR
import keypoints_ref as KR
import test_keypoints_grid_host as TH
from gcslam import _lib as L
from gcslam import keypoints as KP
from gcslam import visual as V
from gcslam.camera import PinholeIntrinsics

pytestmark = pytest.mark.gpu

FEATURES = [n for n, _, _ in L.VISFEAT_FEATURE_FIELDS]
RS = 1e-3   # response_soft_scale: the detector's responses are 1e-4 .. 1e-2, so w_resp = r / (r + RS) is not ~0


def all_rows(det, image, cols=KP.GRID_COLUMNS):
    """Every max_keypoints row of one call, downloaded, with .level, .counts and .level_counts."""
    rows, level, words = det.queue(image)
    torch.cuda.synchronize()
    return KP._pyramid_result([r.cpu().numpy() for r in rows], level.cpu().numpy(), words.cpu().tolist(), None, cols)


def device(name, image=None, **over):
    cfg = TH.grid_config(name, **over)
    img = GR.image(name) if image is None else image
    return all_rows(KP._grid_detector_for(cfg, 0, img.shape[0], img.shape[1]), np.array(img))


@pytest.mark.parametrize("name", GR.NAMES)
def test_device_equals_the_restatement(name):
    ref = GR.expected(name)
    K = GR.config(name)["max_keypoints"]
    got = device(name)
    print(f"{name}: counts {got.counts} level_counts {got.level_counts}")
    TH.same_as_ref(got, ref, K, name)
    if GR.image(name).ndim == 3:   # the fixture is rgb: its own grey image gives the same bytes
        TH.same_as_ref(device(name, KR.grey(GR.image(name))), ref, K, (name, "gray"))
    else:                          # the fixture is gray: the same value in three channels is that grey again
        TH.same_as_ref(device(name, np.repeat(np.array(GR.image(name))[:, :, None], 3, 2)), ref, K, (name, "rgb"))


@pytest.mark.parametrize("name", ["ramp_96x64_l3_k48_c16", "ramp_200x150_k256_c16", "tiny_64x48_edge31"])
def test_detect_returns_trimmed_device_tensors(name):
    ref = GR.expected(name)
    got = KP.detect_keypoints_grid(np.array(GR.image(name)), TH.grid_config(name))
    n = ref["counts"][0]
    assert got.counts == ref["counts"] and np.array(got.level_counts, np.int32).tobytes() == ref["level_counts"].tobytes()
    assert len(got) == 3 and all(t.is_cuda and t.shape == (n,) and t.dtype == torch.float32 for t in got)
    assert got.level.is_cuda and got.level.shape == (n,) and got.level.dtype == torch.int32
    for t, k in zip(tuple(got) + (got.level,), TH.ROWS + ("level",)):
        assert t.cpu().numpy().tobytes() == ref[k].tobytes(), (name, k)


def test_two_calls_are_byte_identical():
    for name in ("ramp_vga_k512", "blocks_61x97_l3_k200_c16"):
        a, b = device(name), device(name)
        assert a.counts[0] == GR.config(name)["max_keypoints"]
        TH.same_bytes(a, b)


def test_a_reused_context_keeps_nothing_of_a_larger_frame():
    """vga, then 96 x 64, then 9 x 9 on one context: every level's offset in the packed workspace moves, the ranks
    and second keys of the larger frame lie where the smaller frames' pixels are, and the cell tables shrink."""
    cfg = TH.grid_config("ramp_96x64_l3_k48_c16", max_width=640, max_height=480)
    images = [np.array(GR.image(n)) for n in ("ramp_vga_k512", "ramp_96x64_l3_k48_c16", "dot_9x9_l8")]
    one = KP.GridDetector(cfg)
    reused = [all_rows(one, img) for img in images]
    one.close()
    for img, got in zip(images, reused):
        fresh = KP.GridDetector(cfg)
        TH.same_bytes(got, all_rows(fresh, img))
        fresh.close()
    TH.same_as_ref(reused[1], GR.expected("ramp_96x64_l3_k48_c16"), 48, "96 x 64 after vga")
    assert reused[0].counts[0] == 48 and reused[0].counts[1] > 1000 and reused[2].counts[:2] == (1, 1)


@pytest.mark.parametrize("name", ["ramp_96x64_l3_k48_c16", "blocks_61x97_l3_k200_c16", "dots_64x96_l3_k16_c16"])
def test_a_torch_view_keeps_its_row_pitch(name):
    img = torch.from_numpy(np.array(GR.image(name))).cuda()
    H, W = img.shape[0], img.shape[1]
    wide = torch.full((H, W + 7) + tuple(img.shape[2:]), 255, dtype=torch.uint8, device="cuda")
    wide[:, :W] = img
    view = wide[:, :W]
    assert not view.is_contiguous()
    det = KP.GridDetector(TH.grid_config(name))
    assert det._image(view)[0].data_ptr() == wide.data_ptr()   # passed as it is, rows (W + 7) pixels apart
    got = all_rows(det, view)
    TH.same_bytes(got, all_rows(det, img))
    TH.same_as_ref(got, GR.expected(name), GR.config(name)["max_keypoints"], name)
    det.close()


@pytest.mark.parametrize("name", GR.ONE_CELL_NAMES)
def test_one_cell_without_redistribution_is_the_pyramid_detector(name):
    """G5 on the device: against PyramidDetector, and at one level against KeypointDetector."""
    cfg = GR.config(name)
    img = np.array(GR.image(name))
    pyr = KP.PyramidDetector(KP.PyramidConfig(**{k: cfg[k] for k in TH.TEN}))
    grid = KP.GridDetector(TH.grid_config(name))
    rows, level, words = pyr.queue(img)
    torch.cuda.synchronize()
    want = KP._pyramid_result([r.cpu().numpy() for r in rows], level.cpu().numpy(), words.cpu().tolist())
    TH.same_as_pyramid(all_rows(grid, img), want)
    assert want.counts[0] > 0
    pyr.close()
    grid.close()
    six = {k: cfg[k] for k in TH.SIX}
    one = KP.KeypointDetector(KP.KeypointConfig(**six))
    rows, counts = one.queue(img)
    grid = KP.GridDetector(KP.GridConfig(**dict(six, n_levels=1, cell_size=64, redistribute=False)))
    got = all_rows(grid, img)
    assert list(got.counts[:3]) == counts.cpu().tolist()[:3] and got.counts[3] == 1
    for a, b in zip(rows, got):
        assert a.cpu().numpy().tobytes() == b.tobytes()
    one.close()
    grid.close()


def test_device_entry_refuses_bad_inputs(lib):
    det = KP.GridDetector(KP.GridConfig(max_width=64, max_height=64, max_keypoints=64))
    buf = torch.zeros(4 * 64 + 52, dtype=torch.float32, device="cuda")
    img = torch.zeros((64, 192), dtype=torch.uint8, device="cuda")
    ptrs = [buf[j * 64:].data_ptr() for j in range(4)] + [buf[256:].data_ptr(), buf[260:].data_ptr()]
    for field, value in TH.BAD_INPUTS:
        i = KP._inputs_struct(img.data_ptr(), 1, 192, 32, 32)
        o = L.GcsKeypointGridOutputs(*ptrs)
        setattr(i if hasattr(i, field) else o, field, {33: 65}.get(value, value))
        assert lib.gcs_detect_keypoints_grid(det.h, C.byref(i), C.byref(o)) == -1, (field, value)
        assert lib.gcs_keypoint_grid_last_error(det.h)
    with pytest.raises(ValueError):
        det.detect(torch.zeros((65, 8), dtype=torch.uint8))
    det.close()


# ---- chaining

@pytest.fixture(scope="module")
def frame():
    import test_gpu_visual_features as TV
    LC, depth, _, _ = TV._frame_inputs()
    return LC, depth, np.array(GR.image("ramp_vga_k512"))


def test_extract_runs_the_grid_detector_for_a_grid_config(frame):
    LC, depth, rgb = frame
    cfg = V.VisualFeatureConfig(response_soft_scale=RS)
    gc = KP.GridConfig(max_keypoints=512)
    kp = KP.detect_keypoints_grid(rgb, gc)
    ref = GR.expected("ramp_vga_k512")
    assert kp.counts == ref["counts"] and kp[0].cpu().numpy().tobytes() == ref["u"].tobytes()
    a = V.extract_visual_features(depth, rgb, None, LC.K, config=cfg, keypoint_config=gc)
    b = V.extract_visual_features(depth, rgb, kp, LC.K, config=cfg)   # the grid's result is a valid keypoints argument
    assert a.count == b.count == 512
    for k in FEATURES:
        assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k
    # another detector than the pyramid one ran
    d = V.extract_visual_features(depth, rgb, None, LC.K, config=cfg, keypoint_config=KP.PyramidConfig(max_keypoints=512))
    assert d.count == 512 and d["u"].cpu().numpy().tobytes() != a["u"].cpu().numpy().tobytes()
    f = V.camera_frame_from_rgbd(depth, rgb, None, LC.K, LC.R_BC, LC.T_BC, 100.05, config=cfg, fusion_config=LC.FUSION,
                                 keypoint_config=gc)
    assert f.arrays is None and f.n_features == 512
    for k in FEATURES:
        assert f.device_arrays[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k


def test_c_route_chains_with_the_nan_padding_and_no_wait(lib):
    """gcs_detect_keypoints_grid, then gcs_visual_features with n_keypoints = max_keypoints and the NaN-padded
    arrays, both queued on a side stream with nothing between them: the real keypoints' rows are those of the
    trimmed route, every further row weighs 0."""
    name, cap = "ramp_200x150_k512_c16", 512
    rgb = np.array(GR.image(name))
    H, W = rgb.shape[:2]
    ref = GR.expected(name)
    n = ref["counts"][0]
    assert n == 467 < cap
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    depth = (2.0 + 0.004 * x - 0.002 * y).astype(np.float32)
    K = PinholeIntrinsics(160.0, 160.0, W / 2.0, H / 2.0)
    gcfg = TH.grid_config(name, max_width=256, max_height=256)
    vcfg = V.VisualFeatureConfig(max_features=cap, max_keypoints=cap, response_soft_scale=RS)
    trimmed = KP.detect_keypoints_grid(rgb, gcfg)
    assert trimmed.counts[0] == n
    want = V.extract_visual_features(depth, rgb, trimmed, K, config=vcfg, trim=False)
    assert want.count == n
    want = {k: v.cpu().numpy() for k, v in want.items()}

    gc, vc = KP.grid_config_struct(gcfg), V.config_struct(vcfg)
    gh, vh = C.c_void_p(), C.c_void_p()
    assert lib.gcs_keypoint_grid_ctx_create(C.byref(gc), C.byref(gh)) == 0
    assert lib.gcs_visfeat_ctx_create(C.byref(vc), C.byref(vh)) == 0
    side = torch.cuda.Stream()
    rgb_d, depth_d = torch.from_numpy(rgb).cuda(), torch.from_numpy(depth).cuda()
    kp = torch.full((3, cap), 7.0, dtype=torch.float32, device="cuda")
    level = torch.full((cap,), 99, dtype=torch.int32, device="cuda")
    words = torch.full((52,), -1, dtype=torch.int32, device="cuda")
    arrs = {k: torch.full((cap, w) if w else (cap,), 77, dtype=getattr(torch, dt), device="cuda")
            for k, w, dt in L.VISFEAT_FEATURE_FIELDS}
    torch.cuda.synchronize()   # the inputs above were made on the default stream
    ki = KP._inputs_struct(rgb_d.data_ptr(), 3, rgb_d.stride(0), W, H)
    ko = L.GcsKeypointGridOutputs(kp[0].data_ptr(), kp[1].data_ptr(), kp[2].data_ptr(), level.data_ptr(),
                                  words.data_ptr(), words[4:].data_ptr())
    vi = V._inputs_struct(depth_d.data_ptr(), 0, depth_d.stride(0) * 4, W, H, rgb_d.data_ptr(), rgb_d.stride(0), K, cap,
                          [kp[j].data_ptr() for j in range(3)])
    vo = L.GcsVisfeatOutputs()
    for k, a in arrs.items():
        setattr(vo, k, a.data_ptr())
    assert lib.gcs_keypoint_grid_ctx_set_stream(gh, C.c_void_p(side.cuda_stream)) == 0
    assert lib.gcs_visfeat_ctx_set_stream(vh, C.c_void_p(side.cuda_stream)) == 0
    assert lib.gcs_detect_keypoints_grid(gh, C.byref(ki), C.byref(ko)) == 0, lib.gcs_keypoint_grid_last_error(gh)
    assert lib.gcs_visual_features(vh, C.byref(vi), C.byref(vo)) == 0, lib.gcs_visfeat_last_error(vh)
    side.synchronize()
    assert words.cpu().tolist()[:4] == [n, n, ref["counts"][2], 8] and vo.count == cap
    assert words.cpu().numpy()[4:].tobytes() == ref["level_counts"].tobytes()
    assert level.cpu().numpy()[:n].tobytes() == ref["level"].tobytes() and (level.cpu().numpy()[n:] == -1).all()
    got = {k: a.cpu().numpy() for k, a in arrs.items()}
    for k in FEATURES:
        assert got[k][:n].tobytes() == want[k][:n].tobytes(), k
    assert (got["weight"][n:] == 0).all() and (got["weight"][:n] > 0).any()
    assert lib.gcs_keypoint_grid_ctx_destroy(gh) == 0 and lib.gcs_visfeat_ctx_destroy(vh) == 0
