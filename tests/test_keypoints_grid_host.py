"""CPU tests of the grid keypoint detector: the exported symbols, the defaults, the refused configs and inputs (with
a device number that names no device, so the refusal is shown to come before any device call),
gcs_keypoint_grid_layout and gcs_detect_keypoints_grid_host -- the definition G1-G4 built for the host -- against
tests/keypoints_grid_ref.py's numpy restatement on every fixture, compared as bytes, and what the definition
reduces to (G5) against the pyramid and the level-0 host builds."""

import ctypes as C
import dataclasses
import os
import re

import numpy as np
import pytest

import keypoints_grid_ref as GR
import keypoints_pyramid_ref as PR
import keypoints_ref as KR
from gcslam import _lib as L
from gcslam import keypoints as KP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gcs_keypoint_grid_config_defaults", "gcs_keypoint_grid_ctx_create", "gcs_keypoint_grid_ctx_destroy",
               "gcs_keypoint_grid_last_error", "gcs_keypoint_grid_ctx_set_stream", "gcs_detect_keypoints_grid",
               "gcs_detect_keypoints_grid_host", "gcs_keypoint_grid_layout")
ROWS = ("u", "v", "response")
TEN = [f.name for f in dataclasses.fields(KP.PyramidConfig)]
SIX = [f.name for f in dataclasses.fields(KP.KeypointConfig)]


def grid_config(name, **over):
    cfg = GR.config(name, **over)
    return KP.GridConfig(**dict(cfg, redistribute=bool(cfg["redistribute"])))


def same_as_ref(got, ref, max_keypoints, what):
    """got: all max_keypoints rows (numpy) with .level, .counts, .level_counts; ref: keypoints_grid_ref.detect's."""
    n = ref["counts"][0]
    assert tuple(got.counts) == tuple(ref["counts"]), (what, got.counts, ref["counts"])
    assert np.array(got.level_counts, np.int32).shape == (8, 6), what
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


def same_as_pyramid(grid, pyr):
    """G5: every row and count; level_counts' first four columns are the pyramid's."""
    assert grid.counts == pyr.counts
    assert tuple(c[:4] for c in grid.level_counts) == pyr.level_counts
    for x, y in zip(tuple(grid) + (grid.level,), tuple(pyr) + (pyr.level,)):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()


def host(name, trim=False, **over):
    return KP.detect_keypoints_grid_host(GR.image(name), grid_config(name, **over), trim=trim)


def _call(lib, c, width=16, height=16, channels=1, pitch=16, cap=65536):
    img, rows = np.zeros((32, 96), np.uint8), [np.zeros(cap, np.float32) for _ in range(3)]
    level, counts, lc = np.zeros(cap, np.int32), np.zeros(4, np.int32), np.zeros(48, np.int32)
    i = KP._inputs_struct(img.ctypes.data, channels, pitch, width, height)
    o = L.GcsKeypointGridOutputs(*(r.ctypes.data for r in rows), level.ctypes.data, counts.ctypes.data, lc.ctypes.data)
    keep = (img, rows, level, counts, lc)
    return i, o, keep


def test_symbols_declared_listed_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "gcslam_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int64_t|const char\*)\s+(gcs_\w+)\s*\(", hdr, re.M))
    for name in NEW_SYMBOLS:
        assert name in declared and name in L.SYMBOLS and hasattr(lib, name), name
    assert lib.gcs_keypoint_grid_last_error(None) == b"null keypoint grid context"
    for k in ("GridConfig", "grid_config_struct", "grid_config_defaults", "grid_layout", "GridDetector",
              "detect_keypoints_grid", "detect_keypoints_grid_host"):
        assert hasattr(KP, k), k
    assert issubclass(KP.GridDetector, KP.PyramidDetector)


def test_defaults(lib):
    c = L.GcsKeypointGridConfig()
    assert lib.gcs_keypoint_grid_config_defaults(C.byref(c)) == 0
    table = dict(PR.DEFAULTS, cell_size=32, redistribute=1)
    assert {k: getattr(c, k) for k in table} == table == GR.DEFAULTS and c.device == 0
    assert dataclasses.asdict(KP.GridConfig()) == dict(table, redistribute=True)
    assert KP.GridConfig().redistribute is True
    assert [f.name for f in dataclasses.fields(KP.GridConfig)] == TEN + ["cell_size", "redistribute"]
    assert KP.grid_config_defaults() == KP.GridConfig()
    assert lib.gcs_keypoint_grid_config_defaults(None) == -1
    with pytest.raises(dataclasses.FrozenInstanceError):
        KP.GridConfig().cell_size = 16


BAD_CONFIGS = [("cell_size", 7), ("cell_size", 65), ("cell_size", 0), ("cell_size", -32), ("redistribute", 2),
               ("redistribute", -1),
               # the pyramid's own
               ("fast_threshold", -1), ("fast_threshold", 256), ("edge_threshold", 3), ("max_keypoints", 0),
               ("max_keypoints", 65537), ("max_width", 0), ("max_height", 0), ("harris_k", float("nan")),
               ("harris_k", float("inf")), ("n_levels", 0), ("n_levels", 9), ("scale_den", 0), ("scale_den", 6),
               ("scale_num", 5), ("scale_num", 11), (("scale_num", "scale_den"), (65, 33))]


@pytest.mark.parametrize("field,value", BAD_CONFIGS)
def test_a_bad_config_is_refused_without_a_device(lib, field, value):
    c = L.GcsKeypointGridConfig()
    assert lib.gcs_keypoint_grid_config_defaults(C.byref(c)) == 0
    for f, v in zip(*((field, value) if isinstance(field, tuple) else ((field,), (value,)))):
        setattr(c, f, v)
    c.device = 1 << 20   # no such device: a create that got as far as the device would return GCS_ERR_HIP (-2)
    h = C.c_void_p()
    assert lib.gcs_keypoint_grid_ctx_create(C.byref(c), C.byref(h)) == -1 and not h.value
    i, o, keep = _call(lib, c)
    assert lib.gcs_detect_keypoints_grid_host(C.byref(c), C.byref(i), C.byref(o)) == -1
    out = np.zeros((8, 5), np.int32)
    assert lib.gcs_keypoint_grid_layout(C.byref(c), 16, 16, out.ctypes.data) == -1


@pytest.mark.parametrize("cell,red", [(8, 0), (64, 1), (32, 1), (9, 0)])
def test_a_good_config_reaches_the_device_it_names(lib, cell, red):
    """The counterpart of the refusals: with the same device number a valid config gets past the checks."""
    c = L.GcsKeypointGridConfig()
    assert lib.gcs_keypoint_grid_config_defaults(C.byref(c)) == 0
    c.cell_size, c.redistribute, c.device = cell, red, 1 << 20
    h = C.c_void_p()
    assert lib.gcs_keypoint_grid_ctx_create(C.byref(c), C.byref(h)) == -2 and not h.value


BAD_INPUTS = [("channels", 2), ("channels", 0), ("channels", 4), ("width", 0), ("height", 0), ("width", -3),
              ("width", 33), ("height", 33), ("pitch", 15), ("image", None), ("kp_u", None), ("kp_v", None),
              ("kp_response", None), ("kp_level", None), ("counts", None), ("level_counts", None)]


@pytest.mark.parametrize("field,value", BAD_INPUTS)
def test_bad_inputs_are_refused(lib, field, value):
    c = L.GcsKeypointGridConfig()
    assert lib.gcs_keypoint_grid_config_defaults(C.byref(c)) == 0
    c.max_width = c.max_height = 32
    c.max_keypoints = 64
    c.device = 1 << 20
    i, o, keep = _call(lib, c, cap=64)
    assert lib.gcs_detect_keypoints_grid_host(C.byref(c), C.byref(i), C.byref(o)) == 0   # the call is good as it stands
    setattr(i if hasattr(i, field) else o, field, value)
    assert lib.gcs_detect_keypoints_grid_host(C.byref(c), C.byref(i), C.byref(o)) == -1
    assert lib.gcs_detect_keypoints_grid_host(C.byref(c), None, C.byref(o)) == -1
    assert lib.gcs_detect_keypoints_grid_host(C.byref(c), C.byref(i), None) == -1
    assert lib.gcs_detect_keypoints_grid(None, C.byref(i), C.byref(o)) == -1


def test_python_entry_refuses_bad_images_and_configs():
    with pytest.raises(ValueError):
        KP.detect_keypoints_grid_host(np.zeros((8, 8, 2), np.uint8))
    with pytest.raises(ValueError):
        KP.detect_keypoints_grid_host(np.zeros((0, 8), np.uint8))
    with pytest.raises(ValueError):
        KP.detect_keypoints_grid_host(np.zeros((8, 8), np.uint8), KP.GridConfig(cell_size=7))
    with pytest.raises(ValueError):
        KP.detect_keypoints_grid_host(np.zeros((8, 8), np.uint8), KP.GridConfig(redistribute=2))
    with pytest.raises(ValueError):
        KP.detect_keypoints_grid_host(np.zeros(100, np.uint8), pitch=20, shape=(8, 8, 1))
    with pytest.raises(ValueError):
        KP.grid_layout(KP.GridConfig(cell_size=65), 8, 8)
    with pytest.raises(ValueError):
        KP.grid_layout(KP.GridConfig(), 0, 8)


@pytest.mark.parametrize("name", GR.NAMES)
def test_layout_equals_the_restatement(name):
    cfg = GR.config(name)
    H, W = GR.image(name).shape[:2]
    got = KP.grid_layout(grid_config(name), W, H)
    want = GR.layout(W, H, **cfg)
    assert got.shape == (8, 5) and got.tobytes() == want.tobytes(), (name, got.tolist(), want.tolist())
    assert got[:, :3].tobytes() == KP.pyramid_layout(KP.PyramidConfig(**{k: cfg[k] for k in TEN}), W, H).tobytes()
    assert got[:cfg["n_levels"], 3:].tolist() == [list(g) for g in GR.expected(name)["grid"]]


@pytest.mark.parametrize("W,H,e,cell,want", [(96, 64, 4, 16, (6, 4)), (96, 64, 4, 8, (11, 7)), (72, 72, 4, 64, (1, 1)),
                                             (73, 72, 4, 64, (2, 1)), (64, 48, 31, 32, (0, 0)), (63, 200, 31, 8, (1, 18)),
                                             (62, 200, 31, 8, (0, 0)), (1920, 1080, 31, 8, (233, 128))])
def test_layout_of_level_0_cells(W, H, e, cell, want):
    got = KP.grid_layout(KP.GridConfig(edge_threshold=e, cell_size=cell), W, H)
    assert tuple(got[0, 3:].tolist()) == want == GR.cells(W, H, e, cell)


@pytest.mark.parametrize("name", GR.NAMES)
def test_host_build_equals_the_restatement(name):
    ref = GR.expected(name)   # (asserts the fixture's own condition)
    got = host(name)
    print(f"{name}: counts {got.counts} level_counts {got.level_counts}")
    same_as_ref(got, ref, GR.config(name)["max_keypoints"], name)


@pytest.mark.parametrize("name", [n for n in GR.NAMES if GR.image(n).ndim == 3])
def test_rgb_equals_its_own_grey_image(name):
    a = host(name)
    b = KP.detect_keypoints_grid_host(KR.grey(GR.image(name)), grid_config(name), trim=False)
    same_bytes(a, b)


@pytest.mark.parametrize("name", GR.ONE_CELL_NAMES + GR.EMPTY[:2])
def test_one_cell_without_redistribution_is_the_pyramid_detector(name):
    """G5, first: redistribute = 0 and every level's kept area inside one cell."""
    cfg = GR.config(name)
    assert cfg["redistribute"] == 0
    pyr = KP.detect_keypoints_pyramid_host(GR.image(name), KP.PyramidConfig(**{k: cfg[k] for k in TEN}), trim=False)
    same_as_pyramid(host(name), pyr)


@pytest.mark.parametrize("name", ["blocks_48x64", "noise_48x64", "dot_9x9", "tiny_6x6"])
@pytest.mark.parametrize("K", [4096, 40])
def test_one_cell_and_one_level_is_the_level_0_detector(name, K):
    """G5, second: also n_levels = 1 -- gcs_detect_keypoints' rows and three counts."""
    cfg = dict(KR.config(name), max_keypoints=K)
    a = KP.detect_keypoints_host(KR.image(name), KP.KeypointConfig(**cfg), trim=False)
    b = KP.detect_keypoints_grid_host(KR.image(name), KP.GridConfig(n_levels=1, cell_size=64, redistribute=False, **cfg),
                                      trim=False)
    H, W = KR.image(name).shape[:2]
    assert W - 8 <= 64 and H - 8 <= 64   # the kept area fits one cell
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    n = a.counts[0]
    assert a.counts[:3] == b.counts[:3] and b.counts[3] == 1
    assert b.level_counts[0][:4] == a.counts[:3] + (K,) and b.level_counts[1:] == ((0,) * 6,) * 7
    assert (b.level[:n] == 0).all() and (b.level[n:] == -1).all()


@pytest.mark.parametrize("name,over", [("blocks_61x97_l3_k200_c16", dict(max_keypoints=4096)),
                                       ("blocks_61x97_l3_k200_c16", dict(max_keypoints=4096, cell_size=8, redistribute=0)),
                                       ("ramp_96x64_l3_k48_c16", dict(max_keypoints=2048)),
                                       ("dots_64x96_l3_k16_c16", dict(max_keypoints=512, cell_size=9, redistribute=0))])
def test_quotas_that_hold_every_survivor_give_the_pyramid_detector(name, over):
    """G5, third: s_l <= quota_l on every level, whatever cell_size and redistribute are."""
    cfg = GR.config(name, **over)
    got = host(name, **over)
    assert all(c[1] <= c[3] for c in got.level_counts) and got.counts[0] == got.counts[1] > 0
    pyr = KP.detect_keypoints_pyramid_host(GR.image(name), KP.PyramidConfig(**{k: cfg[k] for k in TEN}), trim=False)
    same_as_pyramid(got, pyr)
    same_as_ref(got, GR.expected(name, **over), cfg["max_keypoints"], (name, over))


def test_two_calls_give_identical_bytes():
    for name in ("ramp_vga_k512", "blocks_61x97_l3_k200_c16", "dots_64x96_l3_k16_c16"):
        same_bytes(host(name), host(name))


@pytest.mark.parametrize("name", ["ramp_96x64_l3_k48_c16", "blocks_61x97_l3_k200_c16", "dot_9x9_l8", "ramp_200x150_k256_c16"])
def test_a_padded_pitch_gives_the_packed_images_bytes(name):
    img = GR.image(name)
    H, W, ch = img.shape[0], img.shape[1], (3 if img.ndim == 3 else 1)
    pitch = W * ch + 13
    buf = np.full(H * pitch, 255, np.uint8)
    buf.reshape(H, pitch)[:, :W * ch] = img.reshape(H, W * ch)
    a = host(name)
    b = KP.detect_keypoints_grid_host(buf, grid_config(name), pitch=pitch, shape=(H, W, ch), trim=False)
    assert a.counts[0] == GR.expected(name)["counts"][0] > 0
    same_bytes(a, b)


def test_the_spare_quota_goes_to_the_finest_levels_first():
    """ramp_200x150: 76 rows of NaN padding without redistribution, none with it."""
    off, on = host("ramp_200x150_k256_c16_off", trim=True), host("ramp_200x150_k256_c16", trim=True)
    assert off.counts[0] == 180 and on.counts[0] == 256 and off.counts[1:] == on.counts[1:]
    assert [c[4] for c in on.level_counts] == [135, 46, 38, 32, 5, 0, 0, 0]
    lv_off, lv_on = np.asarray(off.level), np.asarray(on.level)
    for j in range(3):   # the levels that got nothing more keep their rows
        assert off[j][lv_off >= 1].tobytes() == on[j][lv_on >= 1].tobytes()
    all_of_them = host("ramp_200x150_k512_c16", trim=True)
    assert all_of_them.counts[0] == all_of_them.counts[1] == 467
