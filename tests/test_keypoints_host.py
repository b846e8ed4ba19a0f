"""CPU tests of the keypoint detector: the exported symbols, the defaults, the refused configs and inputs
(with a device number that names no device, so the refusal is shown to come before any device call), and
gcs_detect_keypoints_host -- the kernels' per-pixel math built for the host -- against
tests/keypoints_ref.py's numpy restatement of the definition on every fixture, compared as bytes."""

import ctypes as C
import dataclasses
import os
import re

import numpy as np
import pytest

import keypoints_ref as KR
from gcslam import _lib as L
from gcslam import keypoints as KP
from gcslam import visual as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gcs_keypoint_config_defaults", "gcs_keypoint_ctx_create", "gcs_keypoint_ctx_destroy",
               "gcs_keypoint_last_error", "gcs_keypoint_ctx_set_stream", "gcs_detect_keypoints",
               "gcs_detect_keypoints_host")
ROWS = ("u", "v", "response")
CAPS = (("blocks_61x97", 32), ("blocks_61x97", 1), ("dots_64x96", 16))


def same_as_ref(got, ref, max_keypoints, what):
    """got: all max_keypoints rows (numpy) with .counts; ref: keypoints_ref.detect's result."""
    n = ref["counts"][0]
    assert tuple(got.counts[:3]) == tuple(ref["counts"]) and got.counts[3] == 0, (what, got.counts, ref["counts"])
    for j, k in enumerate(ROWS):
        assert got[j].shape == (max_keypoints,) and got[j].dtype == np.float32, (what, k)
        assert got[j][:n].tobytes() == ref[k].tobytes(), (what, k)
        assert np.isnan(got[j][n:]).all(), (what, k)


def check_cap(got_rows, name, cap):
    """The kept set is the uncapped restatement's top-N under (response desc, raster asc), in raster order."""
    full = KR.expected(name)
    W = KR.image(name).shape[1]
    raster = (full["v"].astype(np.int64) * W + full["u"].astype(np.int64))
    order = sorted(range(len(raster)), key=lambda i: (-float(full["response"][i]), int(raster[i])))
    top = sorted(order[:cap])
    assert len(top) == cap < len(raster)
    u, v, r = (np.asarray(a) for a in got_rows)
    got_raster = v.astype(np.int64) * W + u.astype(np.int64)
    assert len(u) == cap and (np.diff(got_raster) > 0).all()
    assert got_raster.tolist() == raster[top].tolist()
    assert r.tobytes() == full["response"][top].tobytes()
    if name == "dots_64x96":   # one response everywhere: the first 16 lattice points in raster order
        lattice = [(x, y) for y in range(8, 92, 12) for x in range(8, 60, 12)]
        assert list(zip(u.astype(int).tolist(), v.astype(int).tolist())) == lattice[:cap]


def host(name, trim=False, **over):
    return KP.detect_keypoints_host(KR.image(name), KP.KeypointConfig(**KR.config(name, **over)), trim=trim)


def test_symbols_declared_listed_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "gcslam_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int64_t|const char\*)\s+(gcs_\w+)\s*\(", hdr, re.M))
    for name in NEW_SYMBOLS:
        assert name in declared and name in L.SYMBOLS and hasattr(lib, name), name
    assert lib.gcs_abi_version() == 4 and "#define GCS_ABI_VERSION 4" in hdr
    assert lib.gcs_keypoint_last_error(None) == b"null keypoint context"
    import gcslam
    assert gcslam.keypoints is KP


def test_defaults(lib):
    c = L.GcsKeypointConfig()
    assert lib.gcs_keypoint_config_defaults(C.byref(c)) == 0
    table = dict(fast_threshold=20, edge_threshold=31, max_keypoints=4096, max_width=1920, max_height=1080, harris_k=0.04)
    assert {k: getattr(c, k) for k in table} == table and c.device == 0
    assert dataclasses.asdict(KP.KeypointConfig()) == table == KR.DEFAULTS
    assert KP.config_defaults() == KP.KeypointConfig()
    assert lib.gcs_keypoint_config_defaults(None) == -1


def test_visual_config_keeps_its_fields():
    names = [f.name for f in dataclasses.fields(V.VisualFeatureConfig)]
    assert len(names) == 26 and names[0] == "max_features" and names[-1] == "max_keypoints"
    assert [n for n, _ in L.GcsVisfeatConfig._fields_][-2:] == ["max_keypoints", "device"]
    assert len(L.GcsVisfeatConfig._fields_) == 27


@pytest.mark.parametrize("field,value", [("fast_threshold", -1), ("fast_threshold", 256), ("edge_threshold", 3),
                                         ("max_keypoints", 0), ("max_keypoints", 65537), ("max_width", 0),
                                         ("max_height", 0), ("harris_k", float("nan")), ("harris_k", float("inf"))])
def test_a_bad_config_is_refused_without_a_device(lib, field, value):
    c = L.GcsKeypointConfig()
    assert lib.gcs_keypoint_config_defaults(C.byref(c)) == 0
    setattr(c, field, value)
    c.device = 1 << 20   # no such device: a create that got as far as the device would return GCS_ERR_HIP (-2)
    h = C.c_void_p()
    assert lib.gcs_keypoint_ctx_create(C.byref(c), C.byref(h)) == -1 and not h.value
    img, rows, counts = np.zeros((16, 16), np.uint8), [np.zeros(65536, np.float32) for _ in range(3)], np.zeros(4, np.int32)
    i = KP._inputs_struct(img.ctypes.data, 1, 16, 16, 16)
    o = L.GcsKeypointOutputs(*(r.ctypes.data for r in rows), counts.ctypes.data)
    assert lib.gcs_detect_keypoints_host(C.byref(c), C.byref(i), C.byref(o)) == -1


def test_a_good_config_reaches_the_device_it_names(lib):
    """The counterpart of the refusals: with the same device number a valid config gets past the checks."""
    c = L.GcsKeypointConfig()
    assert lib.gcs_keypoint_config_defaults(C.byref(c)) == 0
    c.device = 1 << 20
    h = C.c_void_p()
    assert lib.gcs_keypoint_ctx_create(C.byref(c), C.byref(h)) == -2 and not h.value


BAD_INPUTS = [("channels", 2), ("channels", 0), ("channels", 4), ("width", 0), ("height", 0), ("width", -3),
              ("width", 33), ("height", 33), ("pitch", 15), ("image", None), ("kp_u", None), ("kp_v", None),
              ("kp_response", None), ("counts", None)]


@pytest.mark.parametrize("field,value", BAD_INPUTS)
def test_bad_inputs_are_refused(lib, field, value):
    c = L.GcsKeypointConfig()
    assert lib.gcs_keypoint_config_defaults(C.byref(c)) == 0
    c.max_width = c.max_height = 32
    c.max_keypoints = 64
    c.device = 1 << 20
    img, rows, counts = np.zeros((32, 96), np.uint8), [np.zeros(64, np.float32) for _ in range(3)], np.zeros(4, np.int32)
    i = KP._inputs_struct(img.ctypes.data, 1, 16, 16, 16)
    o = L.GcsKeypointOutputs(*(r.ctypes.data for r in rows), counts.ctypes.data)
    assert lib.gcs_detect_keypoints_host(C.byref(c), C.byref(i), C.byref(o)) == 0   # the call is good as it stands
    setattr(i if hasattr(i, field) else o, field, value)
    assert lib.gcs_detect_keypoints_host(C.byref(c), C.byref(i), C.byref(o)) == -1
    assert lib.gcs_detect_keypoints_host(C.byref(c), None, C.byref(o)) == -1
    assert lib.gcs_detect_keypoints_host(C.byref(c), C.byref(i), None) == -1
    assert lib.gcs_detect_keypoints(None, C.byref(i), C.byref(o)) == -1


def test_an_rgb_row_is_three_bytes_a_pixel(lib):
    c = L.GcsKeypointConfig()
    assert lib.gcs_keypoint_config_defaults(C.byref(c)) == 0
    c.device = 1 << 20
    img, rows, counts = np.zeros((16, 48), np.uint8), [np.zeros(4096, np.float32) for _ in range(3)], np.zeros(4, np.int32)
    o = L.GcsKeypointOutputs(*(r.ctypes.data for r in rows), counts.ctypes.data)
    i = KP._inputs_struct(img.ctypes.data, 3, 48, 16, 16)
    assert lib.gcs_detect_keypoints_host(C.byref(c), C.byref(i), C.byref(o)) == 0
    i.pitch = 47
    assert lib.gcs_detect_keypoints_host(C.byref(c), C.byref(i), C.byref(o)) == -1


def test_python_entry_refuses_bad_images():
    with pytest.raises(ValueError):
        KP.detect_keypoints_host(np.zeros((8, 8, 2), np.uint8))
    with pytest.raises(ValueError):
        KP.detect_keypoints_host(np.zeros((0, 8), np.uint8))
    with pytest.raises(ValueError):
        KP.detect_keypoints_host(np.zeros((8, 8), np.uint8), KP.KeypointConfig(edge_threshold=2))
    with pytest.raises(ValueError):
        KP.detect_keypoints_host(np.zeros(100, np.uint8), pitch=20, shape=(8, 8, 1))


@pytest.mark.parametrize("name", KR.NAMES)
def test_host_build_equals_the_restatement(name):
    ref = KR.expected(name)   # (asserts the fixture's own condition)
    got = host(name)
    same_as_ref(got, ref, 4096, name)
    print(f"{name}: counts {got.counts}")


@pytest.mark.parametrize("name,cap", CAPS)
def test_caps_keep_the_top_n_in_raster_order(name, cap):
    ref = KR.expected(name, max_keypoints=cap)
    got = host(name, max_keypoints=cap)
    same_as_ref(got, ref, cap, (name, cap))
    assert got.counts[0] == cap and got.counts[1] == KR.expected(name)["counts"][1] > cap   # n_survivors unchanged
    check_cap([a[:cap] for a in got], name, cap)


def test_vga_cap_of_512_bites():
    ref = KR.expected("vga", max_keypoints=512)
    assert KR.expected("vga")["counts"][0] > 512
    same_as_ref(host("vga", max_keypoints=512), ref, 512, "vga 512")


@pytest.mark.parametrize("name", KR.RGB)
def test_rgb_equals_its_own_grey_image(name):
    a = host(name)
    b = KP.detect_keypoints_host(KR.grey(KR.image(name)), KP.KeypointConfig(**KR.config(name)), trim=False)
    assert a.counts == b.counts
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("name", ["blocks_61x97", "noise_48x64", "dot_9x9", "wide_130x35"])
def test_a_padded_pitch_gives_the_packed_images_bytes(name):
    img = KR.image(name)
    H, W, ch = img.shape[0], img.shape[1], (3 if img.ndim == 3 else 1)
    pitch = W * ch + 13
    buf = np.full(H * pitch, 255, np.uint8)
    buf.reshape(H, pitch)[:, :W * ch] = img.reshape(H, W * ch)
    a = host(name)
    b = KP.detect_keypoints_host(buf, KP.KeypointConfig(**KR.config(name)), pitch=pitch, shape=(H, W, ch), trim=False)
    assert a.counts == b.counts and a.counts[0] == KR.expected(name)["counts"][0]
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("name", KR.SMALL)
def test_fast_threshold_0_and_255(name):
    same_as_ref(host(name, fast_threshold=0), KR.expected(name, fast_threshold=0), 4096, (name, 0))
    top = host(name, fast_threshold=255)
    same_as_ref(top, KR.expected(name, fast_threshold=255), 4096, (name, 255))
    assert top.counts == (0, 0, 0, 0)


def test_fast_threshold_255_on_vga():
    assert host("vga", fast_threshold=255).counts == (0, 0, 0, 0)


@pytest.mark.parametrize("name", ["blocks_61x97", "noise_48x64", "vga"])
def test_harris_k_0_changes_responses_only(name):
    a, b = host(name, trim=True), host(name, trim=True, harris_k=0.0)
    same_as_ref(host(name, harris_k=0.0), KR.expected(name, harris_k=0.0), 4096, name)
    assert a.counts == b.counts and a.counts[0] == a.counts[1] > 0   # no cap bites
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert a[2].tobytes() != b[2].tobytes() and (b[2] >= a[2]).all()


def test_extract_needs_rgb_to_detect():
    """keypoints=None with rgb=None is refused before anything is loaded or queued."""
    ex = V.VisualFeatureExtractor.__new__(V.VisualFeatureExtractor)
    with pytest.raises(ValueError, match="rgb"):
        V.VisualFeatureExtractor.extract(ex, np.zeros((8, 8), np.float32), None, None, None)
