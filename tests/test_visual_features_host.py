"""CPU tests of the visual feature operator: the exported symbols, the config defaults against the node's
declared parameters, the refused configs, and gcs_visual_features_host (the kernel's per-keypoint math built
for the host) against tests/visual_features_ref.py's restatement of the node on every fixture -- exact where
the value is a decision or a copied input, rtol 1e-12 where it does not depend on the solve, the solve by
its backward error and everything after it from the library's own beta (visual_features_ref.check)."""

import ctypes as C
import dataclasses
import os
import re

import numpy as np
import pytest

import visual_features_ref as VR
from gcslam import _lib as L
from gcslam import visual as V
from gcslam.camera import CameraFrame, PinholeIntrinsics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gcs_visfeat_config_defaults", "gcs_visfeat_ctx_create", "gcs_visfeat_ctx_destroy",
               "gcs_visfeat_last_error", "gcs_visfeat_ctx_set_stream", "gcs_visual_features",
               "gcs_visual_features_host")
FEATURES = [n for n, _, _ in L.VISFEAT_FEATURE_FIELDS]
DIAG = [n for n, _, _ in L.VISFEAT_DIAG_FIELDS]


def host_rows(case, want_diag=True):
    """A case through gcs_visual_features_host, all max_features rows."""
    cfg = V.VisualFeatureConfig(**case["cfg"])
    out = V.visual_features_host(case["depth"], case["rgb"], case["keypoints"], PinholeIntrinsics(*case["intrinsics"]),
                                 config=cfg, want_diag=want_diag, trim=False)
    return out, out.diag, out.count


def test_symbols_declared_listed_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "gcslam_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int64_t|const char\*)\s+(gcs_\w+)\s*\(", hdr, re.M))
    for name in NEW_SYMBOLS:
        assert name in declared and name in L.SYMBOLS and hasattr(lib, name), name
    assert lib.gcs_abi_version() == 4 and "#define GCS_ABI_VERSION 4" in hdr
    assert lib.gcs_visfeat_last_error(None) == b"null visfeat context"


def test_config_defaults_equal_the_nodes_parameters(lib):
    names = [f.name for f in dataclasses.fields(V.VisualFeatureConfig)]
    assert names == list(VR.NODE_DEFAULTS) + ["max_keypoints"]
    c = V.VisualFeatureConfig()
    assert {n: getattr(c, n) for n in VR.NODE_DEFAULTS} == VR.NODE_DEFAULTS and c.max_keypoints == 4096
    assert V.config_defaults() == c   # gcs_visfeat_config_defaults fills the same values
    s = V.config_struct(dataclasses.replace(c, depth_sample_mode="hex", depth_model="quadratic", kappa_min=0.2), 3)
    assert (s.depth_sample_mode, s.depth_model, s.kappa_min, s.device) == (L.VF_HEX, L.VF_DEPTH_QUADRATIC, 0.2, 3)


@pytest.mark.parametrize("field,value", [("quad_fit_radius", 4), ("hex_radius", 33), ("max_features", 0),
                                         ("max_keypoints", 511), ("depth_sample_mode", 4), ("depth_sample_mode", -1),
                                         ("depth_model", 2), ("depth_model", -1)])
def test_create_refuses_a_bad_config_without_a_device(lib, field, value):
    c = L.GcsVisfeatConfig()
    assert lib.gcs_visfeat_config_defaults(C.byref(c)) == 0
    setattr(c, field, value)
    c.device = 1 << 20   # no such device: a create that got as far as the device would return GCS_ERR_HIP (-2)
    h = C.c_void_p()
    assert lib.gcs_visfeat_ctx_create(C.byref(c), C.byref(h)) == -1 and not h.value
    i, o = L.GcsVisfeatInputs(), L.GcsVisfeatOutputs()
    assert lib.gcs_visual_features_host(C.byref(c), C.byref(i), C.byref(o)) == -1


def test_python_config_refuses_unknown_names():
    with pytest.raises(ValueError, match="Unknown depth_sample_mode"):
        V.config_struct(V.VisualFeatureConfig(depth_sample_mode="median7"))
    with pytest.raises(ValueError, match="Unknown depth_model"):
        V.config_struct(V.VisualFeatureConfig(depth_model="cubic"))


def test_host_call_refuses_bad_inputs():
    case = VR.BY_NAME["shape_bowl"]
    K = PinholeIntrinsics(*case["intrinsics"])
    with pytest.raises(ValueError):   # more keypoints than max_keypoints
        V.visual_features_host(case["depth"], None, np.zeros((40, 3), np.float32), K,
                               config=V.VisualFeatureConfig(max_features=8, max_keypoints=32))
    with pytest.raises(ValueError):
        V.visual_features_host(case["depth"], None, case["keypoints"], PinholeIntrinsics(0.0, 20.0, 1.0, 1.0))
    with pytest.raises(ValueError):
        V.visual_features_host(case["depth"], np.zeros((4, 4, 3), np.uint8), case["keypoints"], K)


@pytest.mark.parametrize("name", VR.CASE_NAMES)
def test_host_entry_meets_the_criteria(name):
    case = VR.BY_NAME[name]
    got, diag, count = host_rows(case)
    fig = VR.check(got, diag, count, case, "host")
    print(f"{name}: {count} rows, {fig['n_fit']} fitted, largest residual / bound {fig['residual']:.3f}")


def test_diagnostics_are_optional():
    case = VR.BY_NAME["holes_median3"]
    a, _, _ = host_rows(case)
    b, d, _ = host_rows(case, want_diag=False)
    assert d is None
    for k in FEATURES:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_keypoints_as_an_array_three_arrays_or_triples():
    case = VR.BY_NAME["shape_tilted"]
    K, kp = PinholeIntrinsics(*case["intrinsics"]), case["keypoints"][:3]
    a = V.visual_features_host(case["depth"], None, kp, K)
    b = V.visual_features_host(case["depth"], None, tuple(np.ascontiguousarray(kp[:, j]) for j in range(3)), K)
    c = V.visual_features_host(case["depth"], None, [tuple(float(x) for x in row) for row in kp], K)   # three triples
    assert a.count == b.count == c.count == 3
    for k in FEATURES:
        assert a[k].tobytes() == b[k].tobytes() == c[k].tobytes(), k


def test_fixtures_hold_the_cases_they_are_for():
    """The reference rows themselves: every branch the issue lists is taken by some keypoint."""
    def rows(name):
        return VR.reference(VR.BY_NAME[name])[2]

    med = rows("holes_median3")
    n_depth, n_fit = [r["n_depth"] for r in med], [r["n_fit"] for r in med]
    assert {0, 1, 3, 4, 5, 8, 9} <= set(n_depth) and {5, 6} <= set(n_fit) and max(n_fit) == 25
    assert any(r["z_valid"] and not r["has_mu"] for r in med) and any(not r["z_valid"] for r in med)
    assert any(r["z_valid"] and np.isnan(r["z_var"]) for r in med)          # 1 to 3 values: no variance
    assert any(n % 2 == 0 and n >= 4 for n in n_depth) and any(n % 2 == 1 and n >= 4 for n in n_depth)
    assert any(r["z_var"] == 0.0 for r in med)                               # duplicate values: all equal
    hexr = rows("holes_hex")
    assert any(not r["z_valid"] and r["n_depth"] in (1, 2, 3) for r in hexr)  # valid centre, under 4 taps
    assert any(r["z_valid"] for r in hexr)
    col = rows("collinear_six")
    assert [r["n_fit"] for r in col] == [6, 6, 3] and col[0]["has_mu"] and not col[2]["has_mu"]
    assert np.linalg.cond(col[0]["M"]) > 1e9                                 # the degenerate fit
    got, diag, _ = host_rows(VR.BY_NAME["shape_bowl"])
    assert (got["kappa_app"] == 100.0).any() and (diag["lam_min"][got["has_mu"] == 1] > 0).all()
    got, diag, _ = host_rows(VR.BY_NAME["kappa_min"])
    fit = got["has_mu"] == 1
    np.testing.assert_allclose(got["kappa_app"][fit] / diag["w_ma"][fit], 0.1, rtol=1e-12)   # clamped at kappa_min
    got, diag, _ = host_rows(VR.BY_NAME["shape_dome"])
    fit = got["has_mu"] == 1
    assert (diag["lam_min"][fit] < 0).all() and diag["w_ma"][fit].max() < 1e-3
    got, diag, _ = host_rows(VR.BY_NAME["shape_saddle"])
    assert (diag["lam_min"][got["has_mu"] == 1] < 0).all() and (diag["K"][got["has_mu"] == 1] < 0).all()
    rng = rows("depth_range")
    assert any(r["z_valid"] and r["z_m"] > 80.0 for r in rng) and any(r["z_valid"] and r["z_m"] < 0.05 for r in rng)
    assert any(np.isnan(k[2]) for k in VR.BY_NAME["holes_median3"]["keypoints"])


def test_rounding_is_half_away_from_zero():
    """u, v at k + 0.5 round up, -0.5 rounds to -1 (outside), -0.4 to 0, W - 0.5 to W (outside); the colour's
    pixel is the clamped coordinate's, rounded the same way."""
    depth = (1.0 + 0.01 * np.arange(VR.W * VR.H, dtype=np.float32)).reshape(VR.H, VR.W)
    rgb = VR._rgb(11)
    pts = [(4.5, 6.5), (2.5, 3.5), (-0.5, 5.0), (5.0, -0.5), (-0.4, 5.0), (5.0, -0.4), (VR.W - 0.5, 5.0),
           (5.0, VR.H - 0.5), (VR.W - 0.6, VR.H - 0.6), (3.5, 0.5), (float("nan"), 2.0), (3e9, 2.0)]
    kp = np.array([(u, v, 10.0) for u, v in pts], np.float32)
    out = V.visual_features_host(depth, rgb, kp, PinholeIntrinsics(*VR.INTRINSICS),
                                 config=V.VisualFeatureConfig(depth_sample_mode="nearest"), want_diag=True)
    want_px = [(5, 7), (3, 4), None, None, (0, 5), (5, 0), None, None, (VR.W - 1, VR.H - 1), (4, 1), None, None]
    for j, px in enumerate(want_px):
        assert bool(out.diag["z_valid"][j]) == (px is not None), (j, pts[j])
        if px is not None:
            assert out.diag["z_m"][j] == float(depth[px[1], px[0]]), (j, pts[j])
    col_px = [(5, 7), (3, 4), (0, 5), (5, 0), (0, 5), (5, 0), (VR.W - 1, 5), (5, VR.H - 1), (VR.W - 1, VR.H - 1), (4, 1),
              (VR.W - 1, 2), (VR.W - 1, 2)]   # -0.5 clamps to 0; W - 0.5 clamps to W - 1; NaN clamps to the upper bound
    for j, (x, y) in enumerate(col_px):
        assert out["color"][j].tolist() == (rgb[y, x] / 255.0).tolist(), (j, pts[j])
    assert not out["weight"][[2, 3, 6, 7, 10, 11]].any() and (out["weight"][[0, 1, 4, 5, 8, 9]] > 0).all()


def test_selection_keeps_the_largest_responses_in_input_order():
    cases = {n: host_rows(VR.BY_NAME[f"select_{n}"]) for n in (8, 9, 20)}
    assert cases[8][1]["kp_index"].tolist() == list(range(8)) and cases[8][2] == 8
    assert cases[9][1]["kp_index"].tolist() == list(range(8)) and cases[9][2] == 8        # of the tied 5s the last goes
    assert cases[20][1]["kp_index"].tolist() == [1, 2, 3, 5, 9, 12, 15, 18]               # ties to the lower index
    resp = np.array([1.0, np.nan, 3.0, np.nan, 2.0], np.float32)                           # NaN ranks last
    case = VR.BY_NAME["shape_bowl"]
    kp = np.stack([np.full(5, 8.0, np.float32), np.full(5, 6.0, np.float32), resp], 1)
    out = V.visual_features_host(case["depth"], None, kp, PinholeIntrinsics(*case["intrinsics"]),
                                 config=V.VisualFeatureConfig(max_features=4, max_keypoints=8), want_diag=True)
    assert out.diag["kp_index"].tolist() == [0, 1, 2, 4] and out.count == 4
    assert out["weight"][1] == 0.0 and (out["weight"][[0, 2, 3]] > 0).all()                # a NaN response weighs 0


def test_padded_rows_and_strides():
    """A depth image with a row pitch beyond its width gives the rows of the packed image."""
    case = VR.BY_NAME["holes_median5"]
    K = PinholeIntrinsics(*case["intrinsics"])
    cfg = V.VisualFeatureConfig(**case["cfg"])
    a = V.visual_features_host(case["depth"], case["rgb"], case["keypoints"], K, config=cfg, want_diag=True)
    wide, wide_rgb = np.full((VR.H, VR.W + 5), 7.0, np.float32), np.zeros((VR.H, VR.W + 3, 3), np.uint8)
    wide[:, :VR.W], wide_rgb[:, :VR.W] = case["depth"], case["rgb"]
    kp = [np.ascontiguousarray(case["keypoints"][:, j]) for j in range(3)]
    lib, c = L.load(), V.config_struct(cfg)
    arrs = {n: np.empty((cfg.max_features, w) if w else (cfg.max_features,), dt)
            for n, w, dt in L.VISFEAT_FEATURE_FIELDS + L.VISFEAT_DIAG_FIELDS}
    i = V._inputs_struct(wide.ctypes.data, 0, wide.strides[0], VR.W, VR.H, wide_rgb.ctypes.data, wide_rgb.strides[0], K,
                         len(kp[0]), [k.ctypes.data for k in kp])
    o = L.GcsVisfeatOutputs()
    for n, x in arrs.items():
        setattr(o, n, x.ctypes.data)
    assert lib.gcs_visual_features_host(C.byref(c), C.byref(i), C.byref(o)) == 0 and o.count == a.count
    for n in FEATURES:
        assert arrs[n][:a.count].tobytes() == a[n].tobytes(), n
    for n in DIAG:
        assert arrs[n][:a.count].tobytes() == a.diag[n].tobytes(), n


def test_camera_frame_takes_a_host_dict_unchanged():
    """Host features go through CameraFrame as before (a device dict needs a GPU: tests/test_gpu_visual_features.py)."""
    case = VR.BY_NAME["shape_bowl"]
    K = PinholeIntrinsics(*case["intrinsics"])
    out = V.visual_features_host(case["depth"], None, case["keypoints"], K)
    f = CameraFrame(dict(out), K, np.eye(3), np.zeros(3), 1.5)
    assert f.device_arrays is None and f.n_features == out.count == len(case["keypoints"])
    for k in FEATURES:
        assert np.array_equal(f.arrays[k], out[k], equal_nan=True), k
    assert f.arrays["cov"].shape == (out.count, 9) and f.arrays["has_color"].tolist() == [0] * out.count
    with pytest.raises(ValueError, match="shape"):
        CameraFrame(dict(out, xyz=out["xyz"][:, :2]), K, np.eye(3), np.zeros(3), 1.5)
