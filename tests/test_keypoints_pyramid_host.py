"""CPU tests of the pyramid keypoint detector: the exported symbols, the defaults, the refused configs and inputs
(with a device number that names no device, so the refusal is shown to come before any device call),
gcs_keypoint_pyramid_layout and gcs_detect_keypoints_pyramid_host -- the kernels' math built for the host --
against tests/keypoints_pyramid_ref.py's numpy restatement of the definition on every fixture, compared as bytes."""

import ctypes as C
import dataclasses
import os
import re

import numpy as np
import pytest

import keypoints_pyramid_ref as PR
import keypoints_ref as KR
from gcslam import _lib as L
from gcslam import keypoints as KP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gcs_keypoint_pyramid_config_defaults", "gcs_keypoint_pyramid_ctx_create", "gcs_keypoint_pyramid_ctx_destroy",
               "gcs_keypoint_pyramid_last_error", "gcs_keypoint_pyramid_ctx_set_stream", "gcs_detect_keypoints_pyramid",
               "gcs_detect_keypoints_pyramid_host", "gcs_keypoint_pyramid_layout")
ROWS = ("u", "v", "response")
SIX = [f.name for f in dataclasses.fields(KP.KeypointConfig)]


def same_as_ref(got, ref, max_keypoints, what):
    """got: all max_keypoints rows (numpy) with .level, .counts, .level_counts; ref: keypoints_pyramid_ref.detect's."""
    n = ref["counts"][0]
    assert tuple(got.counts) == tuple(ref["counts"]), (what, got.counts, ref["counts"])
    assert np.array(got.level_counts, np.int32).tobytes() == ref["level_counts"].tobytes(), (what, got.level_counts)
    for j, k in enumerate(ROWS):
        a = np.asarray(got[j])
        assert a.shape == (max_keypoints,) and a.dtype == np.float32, (what, k)
        assert a[:n].tobytes() == ref[k].tobytes(), (what, k)
        assert np.isnan(a[n:]).all(), (what, k)
    lv = np.asarray(got.level)
    assert lv.shape == (max_keypoints,) and lv.dtype == np.int32, what
    assert lv[:n].tobytes() == ref["level"].tobytes() and (lv[n:] == -1).all(), what


def same_bytes(a, b):
    assert a.counts == b.counts and a.level_counts == b.level_counts
    for x, y in zip(tuple(a) + (a.level,), tuple(b) + (b.level,)):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()


def host(name, trim=False, **over):
    return KP.detect_keypoints_pyramid_host(PR.image(name), KP.PyramidConfig(**PR.config(name, **over)), trim=trim)


def _call(lib, c, width=16, height=16, channels=1, pitch=16, cap=65536):
    img, rows = np.zeros((32, 96), np.uint8), [np.zeros(cap, np.float32) for _ in range(3)]
    level, counts, lc = np.zeros(cap, np.int32), np.zeros(4, np.int32), np.zeros(32, np.int32)
    i = KP._inputs_struct(img.ctypes.data, channels, pitch, width, height)
    o = L.GcsKeypointPyramidOutputs(*(r.ctypes.data for r in rows), level.ctypes.data, counts.ctypes.data, lc.ctypes.data)
    keep = (img, rows, level, counts, lc)
    return i, o, keep


def test_symbols_declared_listed_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "gcslam_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int64_t|const char\*)\s+(gcs_\w+)\s*\(", hdr, re.M))
    for name in NEW_SYMBOLS:
        assert name in declared and name in L.SYMBOLS and hasattr(lib, name), name
    assert lib.gcs_abi_version() == 4 and "#define GCS_ABI_VERSION 4" in hdr
    assert lib.gcs_keypoint_pyramid_last_error(None) == b"null keypoint pyramid context"
    assert [f.name for f in dataclasses.fields(KP.KeypointConfig)] == SIX and len(SIX) == 6


def test_defaults(lib):
    c = L.GcsKeypointPyramidConfig()
    assert lib.gcs_keypoint_pyramid_config_defaults(C.byref(c)) == 0
    table = dict(KR.DEFAULTS, n_levels=8, scale_num=6, scale_den=5)
    assert {k: getattr(c, k) for k in table} == table and c.device == 0
    assert dataclasses.asdict(KP.PyramidConfig()) == table == PR.DEFAULTS
    assert [f.name for f in dataclasses.fields(KP.PyramidConfig)] == SIX + ["n_levels", "scale_num", "scale_den"]
    assert KP.pyramid_config_defaults() == KP.PyramidConfig()
    assert lib.gcs_keypoint_pyramid_config_defaults(None) == -1
    with pytest.raises(dataclasses.FrozenInstanceError):
        KP.PyramidConfig().n_levels = 2


BAD_CONFIGS = [("fast_threshold", -1), ("fast_threshold", 256), ("edge_threshold", 3), ("max_keypoints", 0),
               ("max_keypoints", 65537), ("max_width", 0), ("max_height", 0), ("harris_k", float("nan")),
               ("harris_k", float("inf")), ("n_levels", 0), ("n_levels", 9), ("scale_den", 0), ("scale_den", 6),
               ("scale_den", 7), ("scale_num", 5), ("scale_num", 11), ("scale_num", -6),
               (("scale_num", "scale_den"), (65, 33)), (("scale_num", "scale_den"), (66, 64))]


@pytest.mark.parametrize("field,value", BAD_CONFIGS)
def test_a_bad_config_is_refused_without_a_device(lib, field, value):
    c = L.GcsKeypointPyramidConfig()
    assert lib.gcs_keypoint_pyramid_config_defaults(C.byref(c)) == 0
    for f, v in zip(*((field, value) if isinstance(field, tuple) else ((field,), (value,)))):
        setattr(c, f, v)
    c.device = 1 << 20   # no such device: a create that got as far as the device would return GCS_ERR_HIP (-2)
    h = C.c_void_p()
    assert lib.gcs_keypoint_pyramid_ctx_create(C.byref(c), C.byref(h)) == -1 and not h.value
    i, o, keep = _call(lib, c)
    assert lib.gcs_detect_keypoints_pyramid_host(C.byref(c), C.byref(i), C.byref(o)) == -1
    out = np.zeros((8, 3), np.int32)
    assert lib.gcs_keypoint_pyramid_layout(C.byref(c), 16, 16, out.ctypes.data) == -1


@pytest.mark.parametrize("num,den", [(6, 5), (2, 1), (64, 32), (64, 63), (3, 2)])
def test_a_good_config_reaches_the_device_it_names(lib, num, den):
    """The counterpart of the refusals: with the same device number a valid config gets past the checks."""
    c = L.GcsKeypointPyramidConfig()
    assert lib.gcs_keypoint_pyramid_config_defaults(C.byref(c)) == 0
    c.scale_num, c.scale_den, c.device = num, den, 1 << 20
    h = C.c_void_p()
    assert lib.gcs_keypoint_pyramid_ctx_create(C.byref(c), C.byref(h)) == -2 and not h.value


BAD_INPUTS = [("channels", 2), ("channels", 0), ("channels", 4), ("width", 0), ("height", 0), ("width", -3),
              ("width", 33), ("height", 33), ("pitch", 15), ("image", None), ("kp_u", None), ("kp_v", None),
              ("kp_response", None), ("kp_level", None), ("counts", None), ("level_counts", None)]


@pytest.mark.parametrize("field,value", BAD_INPUTS)
def test_bad_inputs_are_refused(lib, field, value):
    c = L.GcsKeypointPyramidConfig()
    assert lib.gcs_keypoint_pyramid_config_defaults(C.byref(c)) == 0
    c.max_width = c.max_height = 32
    c.max_keypoints = 64
    c.device = 1 << 20
    i, o, keep = _call(lib, c, cap=64)
    assert lib.gcs_detect_keypoints_pyramid_host(C.byref(c), C.byref(i), C.byref(o)) == 0   # the call is good as it stands
    setattr(i if hasattr(i, field) else o, field, value)
    assert lib.gcs_detect_keypoints_pyramid_host(C.byref(c), C.byref(i), C.byref(o)) == -1
    assert lib.gcs_detect_keypoints_pyramid_host(C.byref(c), None, C.byref(o)) == -1
    assert lib.gcs_detect_keypoints_pyramid_host(C.byref(c), C.byref(i), None) == -1
    assert lib.gcs_detect_keypoints_pyramid(None, C.byref(i), C.byref(o)) == -1


def test_python_entry_refuses_bad_images_and_configs():
    with pytest.raises(ValueError):
        KP.detect_keypoints_pyramid_host(np.zeros((8, 8, 2), np.uint8))
    with pytest.raises(ValueError):
        KP.detect_keypoints_pyramid_host(np.zeros((0, 8), np.uint8))
    with pytest.raises(ValueError):
        KP.detect_keypoints_pyramid_host(np.zeros((8, 8), np.uint8), KP.PyramidConfig(n_levels=9))
    with pytest.raises(ValueError):
        KP.detect_keypoints_pyramid_host(np.zeros(100, np.uint8), pitch=20, shape=(8, 8, 1))
    with pytest.raises(ValueError):
        KP.pyramid_layout(KP.PyramidConfig(scale_num=5), 8, 8)
    with pytest.raises(ValueError):
        KP.pyramid_layout(KP.PyramidConfig(), 0, 8)


@pytest.mark.parametrize("name", PR.NAMES)
def test_layout_equals_the_restatement(name):
    cfg = PR.config(name)
    H, W = PR.image(name).shape[:2]
    got = KP.pyramid_layout(KP.PyramidConfig(**cfg), W, H)
    n = cfg["n_levels"]
    assert got[:n, :2].tolist() == [list(s) for s in PR.level_sizes(W, H, n, cfg["scale_num"], cfg["scale_den"])]
    assert got[:n, 2].tolist() == PR.quotas(cfg["max_keypoints"], n, cfg["scale_num"], cfg["scale_den"])
    assert (got[n:] == 0).all() and got[:, 2].sum() == cfg["max_keypoints"]


@pytest.mark.parametrize("W,H,K,n,num,den", [(1920, 1080, 4096, 8, 6, 5), (1 << 28, 1, 65536, 8, 64, 63), (1, 1 << 28, 1, 8, 2, 1),
                                             (16384, 16384, 7, 8, 64, 33), (640, 480, 500, 5, 3, 2), (17, 31, 9, 2, 7, 5)])
def test_layout_at_the_ranges_ends(W, H, K, n, num, den):
    """Python integers against the library's: W D passes 2^63 at the largest widths and denominators."""
    got = KP.pyramid_layout(KP.PyramidConfig(max_keypoints=K, n_levels=n, scale_num=num, scale_den=den), W, H)
    assert got[:n, :2].tolist() == [list(s) for s in PR.level_sizes(W, H, n, num, den)]
    assert got[:n, 2].tolist() == PR.quotas(K, n, num, den)


@pytest.mark.parametrize("name", PR.NAMES)
def test_host_build_equals_the_restatement(name):
    ref = PR.expected(name)   # (asserts the fixture's own condition)
    got = host(name)
    same_as_ref(got, ref, PR.config(name)["max_keypoints"], name)
    print(f"{name}: counts {got.counts} level_counts {got.level_counts}")


@pytest.mark.parametrize("name", [n for n in PR.NAMES if PR.image(n).ndim == 3 and n != "big_1024x704"])
def test_rgb_equals_its_own_grey_image(name):
    a = host(name)
    b = KP.detect_keypoints_pyramid_host(KR.grey(PR.image(name)), KP.PyramidConfig(**PR.config(name)), trim=False)
    same_bytes(a, b)


@pytest.mark.parametrize("name", KR.NAMES)
def test_one_level_is_the_level_0_detector(name):
    """n_levels = 1: the rows and the three counts of detect_keypoints_host; counts[3] is n_levels, the one quota K."""
    cfg = KR.config(name)
    a = KP.detect_keypoints_host(KR.image(name), KP.KeypointConfig(**cfg), trim=False)
    b = KP.detect_keypoints_pyramid_host(KR.image(name), KP.PyramidConfig(n_levels=1, **cfg), trim=False)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    n = a.counts[0]
    assert a.counts[:3] == b.counts[:3] and b.counts[3] == 1 and a.counts[0] == KR.expected(name)["counts"][0]
    assert b.level_counts[0] == a.counts[:3] + (cfg["max_keypoints"],) and b.level_counts[1:] == ((0, 0, 0, 0),) * 7
    assert (b.level[:n] == 0).all() and (b.level[n:] == -1).all()


@pytest.mark.parametrize("name", PR.NAMES)
def test_level_0_rows_are_the_detector_with_quota_0(name):
    cfg = PR.config(name)
    got = host(name, trim=True)
    q0, n0 = got.level_counts[0][3], got.level_counts[0][0]
    six = {k: cfg[k] for k in SIX}
    if q0 == 0:
        assert n0 == 0
        return
    a = KP.detect_keypoints_host(PR.image(name), KP.KeypointConfig(**dict(six, max_keypoints=q0)))
    assert a.counts[:3] == got.level_counts[0][:3] and (np.asarray(got.level)[:n0] == 0).all()
    for x, y in zip(a, got):
        assert x.tobytes() == y[:n0].tobytes()


@pytest.mark.parametrize("name", ["blocks_64x96_l4_k64", "wide_130x35_l3", "blocks_60x96_l3_s2"])
def test_a_levels_rows_are_the_detector_on_the_level_image(name):
    """Level l's rows: the level-0 detector on I_l as a gray8 image with cap quota_l, with the coordinate map."""
    cfg, ref, got = PR.config(name), PR.expected(name), host(name, trim=True)
    H, W = PR.image(name).shape[:2]
    six = {k: cfg[k] for k in SIX}
    lv = np.asarray(got.level)
    for l in range(1, cfg["n_levels"]):
        Wl, Hl = ref["sizes"][l]
        a = KP.detect_keypoints_host(ref["images"][l], KP.KeypointConfig(**dict(six, max_keypoints=got.level_counts[l][3])))
        assert a.counts[0] == got.level_counts[l][0] > 0
        assert PR.coord(a[0], W, Wl).tobytes() == got[0][lv == l].tobytes()
        assert PR.coord(a[1], H, Hl).tobytes() == got[1][lv == l].tobytes()
        assert a[2].tobytes() == got[2][lv == l].tobytes()


def test_two_calls_give_identical_bytes():
    for name in ("vga_k512", "blocks_61x97_l3", "dots_64x96_l3_k16"):
        same_bytes(host(name), host(name))


@pytest.mark.parametrize("name", ["blocks_61x97_l3", "noise_48x64_l3", "dot_9x9_l8", "wide_130x35_l3", "blocks_60x96_l3_s2"])
def test_a_padded_pitch_gives_the_packed_images_bytes(name):
    img = PR.image(name)
    H, W, ch = img.shape[0], img.shape[1], (3 if img.ndim == 3 else 1)
    pitch = W * ch + 13
    buf = np.full(H * pitch, 255, np.uint8)
    buf.reshape(H, pitch)[:, :W * ch] = img.reshape(H, W * ch)
    a = host(name)
    b = KP.detect_keypoints_pyramid_host(buf, KP.PyramidConfig(**PR.config(name)), pitch=pitch, shape=(H, W, ch), trim=False)
    assert a.counts[0] == PR.expected(name)["counts"][0]
    same_bytes(a, b)


def test_a_quota_of_0_keeps_nothing():
    """K = 3 over 8 levels: the integer shares of levels 1.. are 0, level 0 takes all three."""
    got = host("vga_k512", trim=True, max_keypoints=3)
    assert [c[3] for c in got.level_counts] == PR.quotas(3, 8, 6, 5) == [3, 0, 0, 0, 0, 0, 0, 0]
    assert [c[0] for c in got.level_counts] == [3] + [0] * 7 and all(c[1] > 0 for c in got.level_counts)
    same_as_ref(host("vga_k512", max_keypoints=3), PR.expected("vga_k512", max_keypoints=3), 3, "K = 3")
