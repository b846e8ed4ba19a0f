"""CPU tests of the map renderer: the config dataclasses and projection matrices against the reference's
recorded values, gcs_render_prepare_host (the prepare kernel's per-row math built for the host) against
the fixtures' per-row record, the exported symbols, and tests/render_util.py's numpy restatement of
binning and tile render against the recorded indices and tiles.  Fixtures: tests/golden/render_*.npz,
recorded from the reference by tests/golden/make_render.py."""

import ctypes as C
import dataclasses

import numpy as np
import pytest

import render_util as RU
from gcslam import _lib as L
from gcslam import rendering as R

RENDER_SYMBOLS = ("gcs_render_config_defaults", "gcs_render_ctx_create", "gcs_render_ctx_destroy",
                  "gcs_render_last_error", "gcs_render_ctx_set_stream", "gcs_render_prepare", "gcs_render_prepare_host",
                  "gcs_render_bin_tiles", "gcs_render_tiles", "gcs_render_view")


@pytest.fixture(scope="module")
def ops():
    return RU._npz("render_ops")


def test_render_symbols_exported(lib):
    for name in RENDER_SYMBOLS:
        assert name in L.SYMBOLS and hasattr(lib, name), name
    assert lib.gcs_abi_version() == 4
    assert lib.gcs_render_last_error(None) == b"null render context"


def test_config_defaults_equal_the_reference(ops, lib):
    for cls, key in ((R.SplatRenderingConfig, "splat"), (R.BEVPushforwardConfig, "bev")):
        names = [f.name for f in dataclasses.fields(cls)]
        assert names == [str(n) for n in ops[key + "_names"]]
        c = cls()
        assert [float(getattr(c, n)) for n in names] == ops[key + "_defaults"].tolist()
    assert R.config_defaults() == R.SplatRenderingConfig()   # gcs_render_config_defaults fills the same values


def test_create_rejects_a_bad_config(lib):
    for field, val in (("max_splats_per_tile", 0), ("max_splats_per_tile", L.GCS_RENDER_MAX_CAP + 1), ("eps", 0.0),
                       ("fbm_octaves", -1)):
        c = L.GcsRenderConfig()
        lib.gcs_render_config_defaults(C.byref(c))
        setattr(c, field, val)
        h = C.c_void_p()
        assert lib.gcs_render_ctx_create(C.byref(c), C.byref(h)) == -1 and not h.value, field


def test_oblique_Ps_bev15(ops):
    np.testing.assert_allclose(R.oblique_Ps_bev15(R.BEVPushforwardConfig()), ops["Ps_default"], rtol=1e-15, atol=0)
    n, c, s = ops["Ps_cfg"]
    cfg = R.BEVPushforwardConfig(n_views=int(n), phi_center_deg=float(c), phi_span_deg=float(s))
    np.testing.assert_allclose(R.oblique_Ps_bev15(cfg), ops["Ps_custom"], rtol=1e-15, atol=0)
    np.testing.assert_allclose(R.oblique_Ps_bev15(R.BEVPushforwardConfig(n_views=1, phi_center_deg=33.0)),
                               ops["Ps_one"], rtol=1e-15, atol=0)


def _prepare_host(case, **kw):
    return R.prepare_splats_host(case["positions"], case["covariances"], case["directions"], case["kappas"],
                                 case["colors"], case["valid_mask"], case["P_pix"], case["offsets"], case["view_dirs"],
                                 cfg=RU.splat_config(case), fbm_modulate_scale=case["fbm_modulate_scale"],
                                 fbm_seed=case["fbm_seed"], **kw)


@pytest.mark.parametrize("name", RU.CASES)
def test_prepare_host_matches_the_reference_rows(name):
    case = RU.load_case(name)
    got = _prepare_host(case)
    V, n = case["n_views"], case["kappas"].shape[0]
    assert got["means"].shape == (V, n, 2) and got["Sigmas_inv"].shape == (V, n, 2, 2)
    RU.assert_record(got, case)


def test_prepare_host_fbm_and_intensity(ops):
    """fBm at negative and large coordinates with a non-default config, and kappa modulated by intensity
    (below 0 and above intensity_max included), through the same host rows."""
    xy = ops["fbm_xy"]
    n = xy.shape[0]
    pos = np.concatenate([xy, np.zeros((n, 1))], axis=1)
    cov = np.broadcast_to(np.eye(3), (n, 3, 3))
    one = (np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), np.zeros((1, 2)), np.array([[0.0, 0.0, -1.0]]))
    up = np.broadcast_to(np.array([0.0, 0.0, -1.0]), (n, 3))
    got = R.prepare_splats_host(pos, cov, up, np.ones(n), np.ones((n, 3)), None, *one, fbm_modulate_scale=0.5)
    np.testing.assert_allclose(got["fbm"], ops["fbm_default"], rtol=1e-13, atol=0)
    o, g, seed = ops["fbm_args"]
    cfg = R.SplatRenderingConfig(fbm_octaves=int(o), fbm_gain=float(g))
    got = R.prepare_splats_host(pos, cov, up, np.ones(n), np.ones((n, 3)), None, *one, cfg=cfg, fbm_modulate_scale=0.5,
                                fbm_seed=int(seed))
    np.testing.assert_allclose(got["fbm"], ops["fbm_custom"], rtol=1e-13, atol=0)
    assert ops["fbm_default"].min() >= 0.0 and ops["fbm_default"].max() <= 1.0

    m = ops["vmf_mu"].shape[0]
    scale, imax, kmax = ops["vmf_int_args"]
    cfg = R.SplatRenderingConfig(vmf_intensity_scale=float(scale), vmf_intensity_max=float(imax), vmf_kappa_max=float(kmax))
    view = (one[0], one[1], ops["vmf_v"][None])
    got = R.prepare_splats_host(np.zeros((m, 3)), np.broadcast_to(np.eye(3), (m, 3, 3)), ops["vmf_mu"][:, 0],
                                ops["vmf_kappa"][:, 0], np.full((m, 3), 0.5), None, *view, cfg=cfg,
                                intensity=ops["vmf1_intensity"])
    np.testing.assert_allclose(got["colors"][0], np.clip(0.5 * ops["vmf1_out"], 0, 1)[:, None] * np.ones(3), rtol=1e-9,
                               atol=0)


@pytest.mark.parametrize("name", RU.CASES)
def test_numpy_restatement_matches_the_reference(name):
    case = RU.load_case(name)
    cfg = RU.splat_config(case)
    W, H = case["width"], case["height"]
    # the recorded radii come from eigvalsh; the closed form agrees far inside the fixtures' margins
    valid = case["valid_mask"].astype(bool)
    np.testing.assert_allclose(RU.radii_from_inverse(case["Sigmas_inv"][:, valid], cfg.eps), case["radii"][:, valid],
                               rtol=1e-11, atol=0)
    idx, cnt = RU.bin_tiles_np(case["means"], case["radii"], W, H, cfg.tile_size, cfg.max_splats_per_tile)
    assert np.array_equal(idx, case["tile_indices"]) and np.array_equal(cnt, case["tile_counts"])
    s = case["fbm_modulate_scale"]
    colors = case["shaded"] * (((1.0 - s) + s * case["fbm"])[None, :, None] if s > 0 else 1.0)
    tiles = RU.render_tiles_np(case["means"], case["Sigmas_inv"], case["alphas"], colors, idx, cnt, W, H, cfg.tile_size,
                               cfg.ewa_log_clip)
    np.testing.assert_allclose(tiles, case["tiles"], rtol=1e-12, atol=0)


def test_fixture_scene_has_the_cases_it_is_for():
    main = RU.load_case("main")
    cap = int(main["cfg"]["max_splats_per_tile"])
    cnt = main["tile_counts"]
    assert (cnt == cap).any() and ((cnt > 0) & (cnt < cap)).any()
    assert (RU.load_case("band")["tile_counts"] == 0).any()
    listed = main["tile_indices"][main["tile_indices"] >= 0]
    assert main["valid_mask"][listed].all()                    # invalid rows never appear
    assert not RU.load_case("n0")["tiles"].any()
    assert main["tiles"].shape[1:5] == (2, 3, 32, 32)           # partial tiles on both edges of 80 x 48
