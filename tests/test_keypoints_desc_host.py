"""CPU tests of the keypoint describer and the descriptor matcher: the exported symbols, the defaults, the refused
configs and inputs (with a device number that names no device, so the refusal is shown to come before any device
call), the pattern against its generator, D1's inversion of the detectors' coordinate map, and the host twins
gcs_describe_keypoints_host and gcs_match_descriptors_host against tests/keypoints_desc_ref.py's numpy restatement
of D1-D7 on every fixture, compared as bytes (the informative angle within one float32 ulp, as D4 says)."""

import ctypes as C
import dataclasses
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import keypoints_desc_ref as DR
import keypoints_grid_ref as GR
import keypoints_pyramid_ref as PR
import keypoints_ref as KR
from gcslam import _lib as L
from gcslam import descriptors as D
from gcslam import keypoints as KP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gcs_keypoint_desc_config_defaults", "gcs_keypoint_desc_ctx_create", "gcs_keypoint_desc_ctx_destroy",
               "gcs_keypoint_desc_last_error", "gcs_keypoint_desc_ctx_set_stream", "gcs_describe_keypoints",
               "gcs_describe_keypoints_host", "gcs_brief_pattern", "gcs_match_config_defaults", "gcs_match_ctx_create",
               "gcs_match_ctx_destroy", "gcs_match_last_error", "gcs_match_ctx_set_stream", "gcs_match_descriptors",
               "gcs_match_descriptors_host")


def desc_config(name, **over):
    return D.DescriptorConfig(**dict(DR.fixture(name)[1], **over))


def same_as_ref(got, ref, what):
    """got: a Descriptors of numpy arrays; ref: keypoints_desc_ref.describe's.  Bins and descriptors as bytes; the
    angle within one float32 ulp of the restated value (D4), NaN where the row is invalid."""
    n = len(ref["angle_bin"])
    assert got.desc.shape == (n, 32) and got.desc.dtype == np.uint8, what
    assert got.angle.shape == (n,) and got.angle.dtype == np.float32 and got.angle_bin.dtype == np.int32, what
    assert got.angle_bin.tobytes() == ref["angle_bin"].tobytes(), (what, got.angle_bin, ref["angle_bin"])
    assert got.desc.tobytes() == ref["desc"].tobytes(), what
    valid = ref["angle_bin"] >= 0
    assert np.isnan(got.angle[~valid]).all(), what
    err = np.abs(got.angle[valid].astype(np.float64) - ref["angle"][valid].astype(np.float64))
    print(f"{what}: {int(valid.sum())} of {n} rows valid, angle differs on {int((err > 0).sum())} rows")
    assert (err <= np.spacing(np.abs(ref["angle"][valid])).astype(np.float64)).all(), (what, err.max())


def host(name, **over):
    img, cfg, u, v, level = DR.fixture(name)
    return D.describe_keypoints_host(img, (u, v, None, level), desc_config(name, **over))


def test_symbols_declared_listed_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "gcslam_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int64_t|const char\*)\s+(gcs_\w+)\s*\(", hdr, re.M))
    for name in NEW_SYMBOLS:
        assert name in declared and name in L.SYMBOLS and hasattr(lib, name), name
    assert lib.gcs_keypoint_desc_last_error(None) == b"null keypoint descriptor context"
    assert lib.gcs_match_last_error(None) == b"null match context"
    for k in ("DescriptorConfig", "KeypointDescriber", "describe_keypoints", "describe_keypoints_host", "Descriptors",
              "DescriptorMatcher", "match_descriptors", "match_descriptors_host"):
        assert hasattr(D, k), k
    for k in ("D1.", "D2.", "D3.", "D4.", "D5.", "D6.", "D7."):
        assert k in hdr, k


def test_defaults(lib):
    c = L.GcsKeypointDescConfig()
    assert lib.gcs_keypoint_desc_config_defaults(C.byref(c)) == 0
    assert {k: getattr(c, k) for k in DR.DEFAULTS} == DR.DEFAULTS and c.device == 0
    assert {k: PR.DEFAULTS[k] for k in DR.DEFAULTS} == DR.DEFAULTS   # those of the pyramid config
    assert dataclasses.asdict(D.DescriptorConfig()) == DR.DEFAULTS and D.config_defaults() == D.DescriptorConfig()
    assert lib.gcs_keypoint_desc_config_defaults(None) == -1
    m = L.GcsMatchConfig()
    assert lib.gcs_match_config_defaults(C.byref(m)) == 0 and (m.max_query, m.max_train, m.device) == (4096, 4096, 0)
    assert lib.gcs_match_config_defaults(None) == -1
    assert D.config_like(KP.GridConfig(n_levels=3, max_keypoints=48)) == D.DescriptorConfig(n_levels=3, max_keypoints=48)
    assert D.config_like(KP.KeypointConfig()).n_levels == 1


def test_the_pattern_regenerates_identically(lib):
    got = np.zeros((256, 4), np.int8)
    assert lib.gcs_brief_pattern(got.ctypes.data) == 0 and lib.gcs_brief_pattern(None) == -1
    assert got.astype(np.int64).tobytes() == DR.PATTERN.tobytes()
    a, b = DR.PATTERN[:, :2], DR.PATTERN[:, 2:]
    assert ((a * a).sum(1) <= 169).all() and ((b * b).sum(1) <= 169).all() and (a != b).any(1).all()
    assert len({tuple(r) for r in DR.PATTERN.tolist()}) > 250 and np.abs(DR.PATTERN).max() == 13
    assert open(os.path.join(ROOT, "gc-slam_amd", "csrc", "gcs_brief_pattern.h")).read() == DR.GEN.header_text()
    assert (D.brief_pattern() == got).all()


def test_a_quarter_turn_of_the_table_and_of_the_steering_is_exact():
    for k in range(32):
        C_k, S_k = DR.DIR[k]
        assert tuple(DR.DIR[(k + 8) % 32]) == (-S_k, C_k)
        x, y = DR.steer(DR.PATTERN[:, 0], DR.PATTERN[:, 1], k)
        x8, y8 = DR.steer(DR.PATTERN[:, 0], DR.PATTERN[:, 1], (k + 8) % 32)
        assert (x8 == -y).all() and (y8 == x).all()
        assert np.abs(x).max() <= 13 and np.abs(y).max() <= 13   # the reach of D6: 13 + 2 < 16


BAD_CONFIGS = [("n_levels", 0), ("n_levels", 9), ("scale_den", 0), ("scale_den", 6), ("scale_num", 5), ("scale_num", 11),
               (("scale_num", "scale_den"), (65, 33)), ("max_width", 0), ("max_height", 0), ("max_height", -1),
               (("max_width", "max_height"), (1 << 15, 1 << 14)), ("max_keypoints", 0), ("max_keypoints", 65537)]


@pytest.mark.parametrize("field,value", BAD_CONFIGS)
def test_a_bad_config_is_refused_without_a_device(lib, field, value):
    c = L.GcsKeypointDescConfig()
    assert lib.gcs_keypoint_desc_config_defaults(C.byref(c)) == 0
    for f, v in zip(*((field, value) if isinstance(field, tuple) else ((field,), (value,)))):
        setattr(c, f, v)
    c.device = 1 << 20   # no such device: a create that got as far as the device would return GCS_ERR_HIP (-2)
    h = C.c_void_p()
    assert lib.gcs_keypoint_desc_ctx_create(C.byref(c), C.byref(h)) == -1 and not h.value
    i, k, o, keep = _call()
    assert lib.gcs_describe_keypoints_host(C.byref(c), C.byref(i), C.byref(k), C.byref(o)) == -1


def test_a_good_config_reaches_the_device_it_names(lib):
    c = L.GcsKeypointDescConfig()
    assert lib.gcs_keypoint_desc_config_defaults(C.byref(c)) == 0
    c.device = 1 << 20
    h = C.c_void_p()
    assert lib.gcs_keypoint_desc_ctx_create(C.byref(c), C.byref(h)) == -2 and not h.value
    m = L.GcsMatchConfig(16, 16, 1 << 20)
    assert lib.gcs_match_ctx_create(C.byref(m), C.byref(h)) == -2 and not h.value
    for bad in ((0, 16), (16, 0), (-1, 16), ((1 << 20) + 1, 16), (16, (1 << 20) + 1)):
        m = L.GcsMatchConfig(bad[0], bad[1], 1 << 20)
        assert lib.gcs_match_ctx_create(C.byref(m), C.byref(h)) == -1 and not h.value, bad


def _call(n=4):
    img = np.zeros((48, 144), np.uint8)
    u, v, level = np.full(n, 20, np.float32), np.full(n, 20, np.float32), np.zeros(n, np.int32)
    angle, bins, desc = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros((n, 32), np.uint8)
    i = KP._inputs_struct(img.ctypes.data, 1, 144, 40, 40)
    k = L.GcsKeypointDescKeypoints(n, u.ctypes.data, v.ctypes.data, level.ctypes.data)
    o = L.GcsKeypointDescOutputs(angle.ctypes.data, bins.ctypes.data, desc.ctypes.data)
    return i, k, o, (img, u, v, level, angle, bins, desc)


BAD_INPUTS = [("channels", 2), ("channels", 0), ("width", 0), ("height", 0), ("width", -3), ("width", 49), ("height", 49),
              ("pitch", 39), ("image", None), ("n_keypoints", -1), ("n_keypoints", 9), ("kp_u", None), ("kp_v", None),
              ("kp_angle", None), ("kp_angle_bin", None), ("desc", None)]


@pytest.mark.parametrize("field,value", BAD_INPUTS)
def test_bad_inputs_are_refused(lib, field, value):
    c = L.GcsKeypointDescConfig()
    assert lib.gcs_keypoint_desc_config_defaults(C.byref(c)) == 0
    c.max_width = c.max_height = 48
    c.max_keypoints = 8
    c.device = 1 << 20
    i, k, o, keep = _call()
    assert lib.gcs_describe_keypoints_host(C.byref(c), C.byref(i), C.byref(k), C.byref(o)) == 0   # good as it stands
    k.kp_level = None   # and with every keypoint on level 0
    assert lib.gcs_describe_keypoints_host(C.byref(c), C.byref(i), C.byref(k), C.byref(o)) == 0
    setattr(next(s for s in (i, k, o) if hasattr(s, field)), field, value)
    assert lib.gcs_describe_keypoints_host(C.byref(c), C.byref(i), C.byref(k), C.byref(o)) == -1
    assert lib.gcs_describe_keypoints_host(C.byref(c), None, C.byref(k), C.byref(o)) == -1
    assert lib.gcs_describe_keypoints_host(C.byref(c), C.byref(i), None, C.byref(o)) == -1
    assert lib.gcs_describe_keypoints_host(C.byref(c), C.byref(i), C.byref(k), None) == -1
    assert lib.gcs_describe_keypoints(None, C.byref(i), C.byref(k), C.byref(o)) == -1


def _match_call(n_q=3, n_t=5):
    q, t = np.zeros((n_q, 32), np.uint8), np.zeros((n_t + 1, 32), np.uint8)
    out = np.zeros((3, n_q), np.int32)
    i = L.GcsMatchInputs(n_q, n_t, q.ctypes.data, t.ctypes.data, None, None)
    o = L.GcsMatchOutputs(out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data)
    return i, o, (q, t, out)


@pytest.mark.parametrize("field,value", [("n_query", -1), ("n_query", 9), ("n_train", -1), ("n_train", 9), ("q", None),
                                         ("t", None), ("idx", None), ("dist", None), ("dist2", None), ("q", "odd"),
                                         ("t", "odd")])
def test_bad_match_inputs_are_refused(lib, field, value):
    c = L.GcsMatchConfig(8, 8, 1 << 20)
    i, o, keep = _match_call()
    assert lib.gcs_match_descriptors_host(C.byref(c), C.byref(i), C.byref(o)) == 0
    if value == "odd":
        value = getattr(i, field) + 2   # not 4-byte aligned
    setattr(i if hasattr(i, field) else o, field, value)
    assert lib.gcs_match_descriptors_host(C.byref(c), C.byref(i), C.byref(o)) == -1
    assert lib.gcs_match_descriptors_host(C.byref(c), None, C.byref(o)) == -1
    assert lib.gcs_match_descriptors_host(C.byref(c), C.byref(i), None) == -1
    assert lib.gcs_match_descriptors_host(None, C.byref(i), C.byref(o)) == -1
    assert lib.gcs_match_descriptors(None, C.byref(i), C.byref(o)) == -1


def test_python_entry_refuses_bad_arguments():
    img, u = np.zeros((40, 40), np.uint8), np.full(2, 20, np.float32)
    with pytest.raises(ValueError):
        D.describe_keypoints_host(np.zeros((8, 8, 2), np.uint8), (u, u))
    with pytest.raises(ValueError):
        D.describe_keypoints_host(img, (u, u[:1]))
    with pytest.raises(ValueError):
        D.describe_keypoints_host(img, (u, u), D.DescriptorConfig(n_levels=9))
    with pytest.raises(ValueError):
        D.describe_keypoints_host(img, (u,))
    with pytest.raises(ValueError):
        D.nearest_host(np.zeros((3, 31), np.uint8), np.zeros((3, 32), np.uint8))
    with pytest.raises(ValueError):
        D.nearest_host(np.zeros((3, 32), np.uint8), np.zeros((3, 32), np.uint8), np.zeros(2, np.int32))


# ---- D1: the inversion of the detectors' coordinate map

@pytest.mark.parametrize("name", GR.NAMES)
def test_the_level_pixel_inverts_the_grid_detectors_coordinates(name):
    ref = GR.expected(name)
    H, W = GR.image(name).shape[:2]
    for l, (W_l, H_l) in enumerate(ref["sizes"]):
        if W_l >= 1 and H_l >= 1:   # every pixel of the level, not only the kept ones
            x, y = np.arange(W_l), np.arange(H_l)
            assert (DR.level_pixel(PR.coord(x, W, W_l), W_l, W) == x).all(), (name, l)
            assert (DR.level_pixel(PR.coord(y, H, H_l), H_l, H) == y).all(), (name, l)
    m = ref["level"]
    for l in set(m.tolist()):
        W_l, H_l = ref["sizes"][l]
        x, y = DR.level_pixel(ref["u"][m == l], W_l, W), DR.level_pixel(ref["v"][m == l], H_l, H)
        assert (PR.coord(x, W, W_l) == ref["u"][m == l]).all() and (PR.coord(y, H, H_l) == ref["v"][m == l]).all(), (name, l)


@pytest.mark.parametrize("name", PR.SMALL + ("vga_k512",))
def test_the_level_pixel_inverts_the_pyramid_detectors_coordinates(name):
    ref = PR.expected(name)
    H, W = PR.image(name).shape[:2]
    m = ref["level"]
    for l in set(m.tolist()):
        W_l, H_l = ref["sizes"][l]
        x, y = DR.level_pixel(ref["u"][m == l], W_l, W), DR.level_pixel(ref["v"][m == l], H_l, H)
        assert (PR.coord(x, W, W_l) == ref["u"][m == l]).all() and (PR.coord(y, H, H_l) == ref["v"][m == l]).all(), (name, l)


def test_the_host_twin_sees_the_inverted_pixel():
    """The largest geometry: every column of level 7 of a 1920-wide image, through the host twin's validity."""
    W, H = 1920, 64
    W_l, H_l = PR.level_sizes(W, H, 8, 6, 5)[1]
    x = np.arange(W_l)
    u = PR.coord(x, W, W_l)
    v = np.full(W_l, PR.coord(np.array([20]), H, H_l)[0], np.float32)
    got = D.describe_keypoints_host(np.zeros((H, W), np.uint8), (u, v, None, np.full(W_l, 1, np.int32)))
    assert ((got.angle_bin >= 0) == ((x >= 16) & (x < W_l - 16))).all() and (got.angle_bin >= 0).sum() == W_l - 32


# ---- the host twins against the restatement

@pytest.mark.parametrize("name", DR.NAMES)
def test_host_describer_equals_the_restatement(name):
    same_as_ref(host(name), DR.expected(name), name)


@pytest.mark.parametrize("name", ["ramp_96x64_l3_k48_c16", "blocks_61x97_l3_k200_c16"])
def test_rgb_and_a_padded_pitch_give_the_same_bytes(name):
    img, cfg, u, v, level = DR.fixture(name)
    assert img.ndim == 3
    H, W = img.shape[:2]
    ref = DR.expected(name)
    same_as_ref(D.describe_keypoints_host(KR.grey(img), (u, v, None, level), desc_config(name)), ref, (name, "grey"))
    pitch = 3 * W + 13
    buf = np.full(H * pitch, 255, np.uint8)
    buf.reshape(H, pitch)[:, :3 * W] = img.reshape(H, 3 * W)
    got = D.describe_keypoints_host(buf, (u, v, None, level), desc_config(name), pitch=pitch, shape=(H, W, 3))
    same_as_ref(got, ref, (name, "pitch"))


def test_a_null_level_array_is_level_0():
    img, cfg, u, v, level = DR.fixture("quarter_64")
    assert level is None
    a = host("quarter_64")
    b = D.describe_keypoints_host(img, (u, v, None, np.zeros(len(u), np.int32)), desc_config("quarter_64", n_levels=8))
    assert a.desc.tobytes() == b.desc.tobytes() and a.angle_bin.tobytes() == b.angle_bin.tobytes()


def test_the_detectors_padding_rows_are_invalid():
    name = "ramp_200x150_k512_c16"
    kp = KP.detect_keypoints_grid_host(GR.image(name), KP.GridConfig(**dict(GR.config(name), redistribute=True)), trim=False)
    n = kp.counts[0]
    assert n == 467 and len(kp[0]) == 512
    got = D.describe_keypoints_host(GR.image(name), kp)
    assert (got.angle_bin[n:] == -1).all() and np.isnan(got.angle[n:]).all() and (got.desc[n:] == 0).all()
    assert (got.angle_bin[:n] >= 0).all() and got.desc[:n].any(1).all()   # edge_threshold 31 >= 16: no invalid row
    ref = DR.describe(GR.image(name), kp[0], kp[1], kp.level)
    same_as_ref(got, ref, name)


def test_a_quarter_turn_moves_every_bin_by_8_and_keeps_the_descriptor():
    """np.rot90 puts the pixel (x, y) at (y, N - 1 - x): an offset (dx, dy) becomes (dy, -dx), so m10' = m01 and
    m01' = -m10, and m10' C_k + m01' S_k = m10 C_{k+8} + m01 S_{k+8}: the turned keypoint's bin is bin - 8 mod 32.
    The steered pattern turns with it exactly (D5), the box is symmetric, so the 256 bits are the same.  The fixture's
    condition check asserts that no keypoint ties in D3's argmax, the one place where the turn is not exact."""
    a, b = host("quarter_64"), host("quarter_64_turned")
    same_as_ref(a, DR.expected("quarter_64"), "quarter_64")
    assert (a.angle_bin >= 0).all() and len(a) == 13
    assert (b.angle_bin == (a.angle_bin - 8) % 32).all(), (a.angle_bin, b.angle_bin)
    assert a.desc.tobytes() == b.desc.tobytes() and a.desc.any()
    assert not (a.desc == DR.expected("centre_33x33")["desc"][0]).all(1).any()


@pytest.mark.parametrize("name", DR.MATCH_NAMES)
def test_host_matcher_equals_the_restatement(name):
    q, t, q_bin, t_bin = DR.match_fixture(name)
    want = DR.match_expected(name)
    got = D.nearest_host(q, t, q_bin, t_bin)
    for g, w, k in zip(got, want, ("idx", "dist", "dist2")):
        assert g.dtype == np.int32 and g.tobytes() == w.tobytes(), (name, k)


def test_match_descriptors_host_applies_the_filters():
    a, b = DR.expected("ramp_96x64_l3_k48_c16"), DR.expected("blocks_61x97_l3_k200_c16")
    da, db = (D.Descriptors(r["desc"], r["angle"], r["angle_bin"]) for r in (a, b))
    for kw in (dict(), dict(max_distance=256, ratio=(1, 1), cross_check=False), dict(cross_check=False), dict(ratio=(9, 10))):
        got, want = D.match_descriptors_host(da, db, **kw), DR.match_filtered(a, b, **kw)
        for g, w in zip(got, want):
            assert g.tobytes() == w.tobytes(), kw
    all_of_them = D.match_descriptors_host(da, da)
    assert (all_of_them[0] == all_of_them[1]).all() and (all_of_them[2] == 0).all() and len(all_of_them[0]) > 40
    assert len(D.match_descriptors_host(da, db, max_distance=None, ratio=None, cross_check=False)[0]) == 48   # filters off


def test_the_restated_end_to_end_pair_meets_its_figures():
    ia, ib, dist, both0, exact = DR.vga_pair_matches()
    assert (np.diff(ia) > 0).all() and (dist <= 64).all() and both0.sum() >= 1
    assert len(DR.vga_pyramid_pair()[2]) == DR.VGA_PYRAMID_PAIRS


def test_the_generator_checks_the_committed_header():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_brief_pattern.py"), "--check"], capture_output=True)
    assert r.returncode == 0, r.stdout
