"""GPU tests of the map renderer (gcslam.rendering, csrc/gcs_render.hip) against the fixtures recorded from
the reference (tests/golden/render_*.npz): every operator and every kernel on the fixture's own stage
inputs, render_map_view end to end on the fixture scenes, bitwise reproducibility on a clustered input,
larger shapes against tests/render_util.py's numpy restatement (itself held to the fixtures by
test_rendering_host.py), and a render of a live map.

Bars (element-wise): per-row quantities and tile images on recorded stage inputs at rtol 1e-9 (atol 1e-12 on images),
the project's bar for routes without an eigenvector; fBm at 1e-13; end-to-end images at rtol 1e-7 with
atol 1e-7, test_gpu_surfels.py's bar for quantities that pass through a small inverse; indices and
counts equal."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import render_util as RU
from gcslam import rendering as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
cpu = lambda x: x.detach().cpu().numpy()  # noqa: E731
up = lambda a: torch.tensor(np.asarray(a), device=DEV)  # noqa: E731


@pytest.fixture(scope="module")
def ops():
    return RU._npz("render_ops")


# ---------------------------------------------------------------------- per-element operators
def test_pushforward_rotation_opacity(ops):
    mu2, S2 = R.pushforward_gaussians_3d_to_2d(up(ops["pf_mu"]), up(ops["pf_Sigma"]), ops["pf_P"])
    assert tuple(mu2.shape) == (4, 64, 2) and tuple(S2.shape) == (4, 64, 2, 2)
    np.testing.assert_allclose(cpu(mu2), ops["pf_mu2"], rtol=1e-9, atol=0)
    np.testing.assert_allclose(cpu(S2), ops["pf_S2"], rtol=1e-9, atol=0)
    np.testing.assert_allclose(cpu(R.rotate_vmf_etas(ops["rot_R"], up(ops["rot_etas"]))), ops["rot_out"], rtol=1e-9,
                               atol=0)
    np.testing.assert_allclose(cpu(R.opacity_from_logdet(up(ops["op_logdet"]))), ops["op_default"], rtol=1e-9, atol=0)
    g, l0, am = ops["op_args"]
    np.testing.assert_allclose(cpu(R.opacity_from_logdet(up(ops["op_logdet"]), g, l0, am)), ops["op_custom"], rtol=1e-9,
                               atol=0)


def test_vmf_shading_multi_lobe(ops):
    v, mu, k = ops["vmf_v"], up(ops["vmf_mu"]), up(ops["vmf_kappa"])
    mu0 = mu.clone()
    np.testing.assert_allclose(cpu(R.vmf_shading_multi_lobe(v, mu, k)), ops["vmf_plain"], rtol=1e-9, atol=0)
    np.testing.assert_allclose(cpu(R.vmf_shading_multi_lobe(v, mu, k, pi_b=ops["vmf_pi"])), ops["vmf_pi_out"], rtol=1e-9,
                               atol=0)
    scale, imax, kmax = ops["vmf_int_args"]
    got = R.vmf_shading_multi_lobe(v, mu, k, pi_b=ops["vmf_pi"], intensity=up(ops["vmf_intensity"]),
                                   intensity_scale=float(scale), intensity_max=float(imax), kappa_max=float(kmax))
    np.testing.assert_allclose(cpu(got), ops["vmf_int_out"], rtol=1e-9, atol=0)
    assert not np.allclose(ops["vmf_int_out"], ops["vmf_pi_out"], rtol=1e-3)   # the modulation does something
    assert torch.equal(mu, mu0)                                                # and the lobes are left alone


def test_fbm_at_splat_positions(ops):
    np.testing.assert_allclose(cpu(R.fbm_at_splat_positions(up(ops["fbm_xy"]))), ops["fbm_default"], rtol=1e-13, atol=0)
    o, g, seed = ops["fbm_args"]
    np.testing.assert_allclose(cpu(R.fbm_at_splat_positions(up(ops["fbm_xy"]), int(o), float(g), int(seed))),
                               ops["fbm_custom"], rtol=1e-13, atol=0)


# ---------------------------------------------------------------------- the kernels, stage by stage
@pytest.mark.parametrize("name", RU.CASES)
def test_prepare_kernel(name):
    case = RU.load_case(name)
    r = R.renderer_for(RU.splat_config(case))
    got = r.prepare(case["positions"], case["covariances"], case["directions"], case["kappas"], case["colors"],
                    case["valid_mask"], case["P_pix"], case["offsets"], case["view_dirs"],
                    fbm_modulate_scale=case["fbm_modulate_scale"], fbm_seed=case["fbm_seed"])
    RU.assert_record({k: cpu(v) for k, v in got.items()}, case)


@pytest.mark.parametrize("name", RU.CASES)
def test_bin_kernel_on_recorded_inputs(name):
    """The reference's own call: the valid rows' means and Sigma^-1 in order; indices count those rows."""
    case = RU.load_case(name)
    cfg = RU.splat_config(case)
    rows = np.flatnonzero(case["valid_mask"])
    idx, cnt = R.splat_indices_for_tiles(up(case["means"][:, rows]), up(case["Sigmas_inv"][:, rows]), case["width"],
                                         case["height"], cfg.tile_size, cfg.max_splats_per_tile, cfg.eps)
    assert idx.dtype == torch.int32 and cnt.dtype == torch.int32
    idx, cnt = cpu(idx), cpu(cnt)
    got = np.where(idx >= 0, rows[np.maximum(idx, 0)] if rows.size else -1, -1)
    assert np.array_equal(cnt, case["tile_counts"])
    assert np.array_equal(got, case["tile_indices"])


@pytest.mark.parametrize("name", RU.CASES)
def test_render_kernel_on_recorded_inputs(name):
    case = RU.load_case(name)
    cfg = RU.splat_config(case)
    tiles = R.render_tiles_ewa(up(case["means"]), up(case["Sigmas_inv"]), up(case["alphas"]), up(case["shaded"]),
                               up(case["tile_indices"]), up(case["tile_counts"]), case["width"], case["height"],
                               cfg.tile_size, cfg.ewa_log_clip, means_world_xy=up(case["positions"][:, :2]),
                               fbm_octaves=cfg.fbm_octaves, fbm_gain=cfg.fbm_gain, fbm_seed=case["fbm_seed"],
                               fbm_modulate_scale=case["fbm_modulate_scale"])
    assert tuple(tiles.shape) == case["tiles"].shape
    np.testing.assert_allclose(cpu(tiles), case["tiles"], rtol=1e-9, atol=1e-12)


# ---------------------------------------------------------------------- end to end
@pytest.mark.parametrize("name", RU.CASES)
def test_render_map_view_end_to_end(name):
    case = RU.load_case(name)
    W, H = case["width"], case["height"]
    res = R.render_map_view(RU.device_view(case), bev=R.BEVPushforwardConfig(n_views=case["n_views"]),
                            cfg=RU.splat_config(case), width=W, height=H, pixels_per_metre=case["pixels_per_metre"],
                            centre_xy=case["centre_xy"], fbm_modulate_scale=case["fbm_modulate_scale"],
                            fbm_seed=case["fbm_seed"])
    idx, cnt, img = cpu(res.tile_indices), cpu(res.tile_counts), cpu(res.images)
    assert np.array_equal(cnt, case["tile_counts"]) and np.array_equal(idx, case["tile_indices"])
    assert img.shape == (case["n_views"], H, W, 3) and img.dtype == np.float64
    np.testing.assert_allclose(img, RU.image_from_tiles(case["tiles"], W, H), rtol=1e-7, atol=1e-7)
    assert case["valid_mask"][idx[idx >= 0]].all()           # invalid rows are never listed
    if name == "n0":
        assert not img.any() and not cnt.any()
    else:
        assert img.any()


# ---------------------------------------------------------------------- determinism and larger shapes
_scene = RU.random_scene


def test_two_calls_are_bitwise_equal():
    """Every row inside one tile, a quarter of them bit-identical copies: the order in which the bin
    kernel's waves append cannot reach the result."""
    rng = np.random.default_rng(5)
    sc = _scene(rng, 3000, [((40.0, 24.0), 3000)], 3.0, 96, 64)
    for k in ("positions", "covariances", "directions", "kappas", "colors"):
        sc[k][750:1500] = sc[k][:750]
    view = RU.device_view(sc)
    kw = dict(bev=R.BEVPushforwardConfig(n_views=2), cfg=R.SplatRenderingConfig(max_splats_per_tile=48), width=96,
              height=64, pixels_per_metre=1.0, centre_xy=(0.0, 0.0), fbm_modulate_scale=0.1)
    a = R.render_map_view(view, **kw)
    b = R.render_map_view(view, **kw)
    for f in ("images", "tile_indices", "tile_counts"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    assert int(a.tile_counts.max()) == 48 and a.images.any()


_check_against_restatement = RU.check_against_restatement


def test_n4097_two_clusters_in_one_tile_cap64():
    rng = np.random.default_rng(6)
    sc = _scene(rng, 4097, [((42.0, 40.0), 300), ((54.0, 52.0), 300)], 2.0, 96, 72)   # both in tile (1, 1)
    cnt = _check_against_restatement(sc, R.SplatRenderingConfig(max_splats_per_tile=64), 1, 96, 72)
    assert cnt[0, 1, 1] == 64 and cnt.min() >= 0


def test_n300_cap_above_n_keeps_every_row():
    rng = np.random.default_rng(7)
    sc = _scene(rng, 300, [((16.0, 16.0), 300)], 4.0, 40, 40)
    sc["valid_mask"][:] = True
    cnt = _check_against_restatement(sc, R.SplatRenderingConfig(max_splats_per_tile=512), 1, 40, 40)
    assert cnt[0, 0, 0] == 300


@pytest.mark.parametrize("cap", [64, 1024])
def test_every_row_overlaps_every_tile(cap):
    """4097 rows whose radius covers the whole image, ordered so that each is nearer to tile (0, 0)'s centre
    than all before it: nothing is filtered there, and the kept list is rebuilt over and over."""
    rng = np.random.default_rng(8)
    n, W, H = 4097, 70, 40
    d = np.sort(rng.uniform(1.0, 30.0, n))[::-1]
    th = rng.uniform(0.0, 2.0 * np.pi, n)
    means = np.stack([16.0 + d * np.cos(th), 16.0 + d * np.sin(th)], 1)[None].copy()
    means[0, 100] = means[0, 50]                      # one exact tie
    radii = np.full((1, n), 1.0e3)
    r = R.renderer_for(R.SplatRenderingConfig(max_splats_per_tile=cap))
    idx, cnt = r.bin_tiles(up(means), None, W, H, radii=up(radii))
    ref_idx, ref_cnt = RU.bin_tiles_np(means, radii, W, H, 32, cap)
    assert np.array_equal(cpu(cnt), ref_cnt) and np.array_equal(cpu(idx), ref_idx)
    assert (ref_cnt == min(cap, n)).all()


# ---------------------------------------------------------------------- a live map
def test_render_from_a_live_map():
    from gcslam import association as GA, primitive_map as gpm, synthetic
    from gcslam.surfels import SurfelExtractionConfig, extract_lidar_surfels
    am = gpm.AtlasMap(m_tile=4096, max_tiles=64, max_merge=0)
    scfg = SurfelExtractionConfig(n_surfel=1024, n_feat=512)
    for k in range(2):
        sc = synthetic.make_scan(8192, 40 + k)
        z = np.array([0.1 * k, 0.04 * k, 0.0, 0.0, 0.0, 0.02 * k])
        pts, ts, ws = (torch.as_tensor(sc[f], device=DEV) for f in ("points", "timestamps", "weights"))
        batch, _, _ = extract_lidar_surfels(pts, ts, ws, config=scfg)
        active = gpm.ma_hex_stencil_tile_ids(z[:3], 2.0, 1, 1)
        gpm.primitive_map_recency_inflate(am, active, 10 + k)
        view = gpm.extract_atlas_map_view(am, active, 1024)
        res, _, _ = GA.associate_primitives_ot(batch, view, GA.AssociationConfig(scan_seq=10 + k, r_stencil_tiles_z=1))
        gpm.primitive_map_update(am, batch, res, z, active, float(sc["scan_end_time"]), 10 + k)
    kw = dict(bev=R.BEVPushforwardConfig(n_views=3), width=160, height=120, pixels_per_metre=12.0,
              centre_xy=(float(z[0]), float(z[1])))
    view = gpm.extract_atlas_map_view(am, active, 1024)
    n_valid = int(view.valid_mask.sum())
    assert n_valid > 100
    a = R.render_map_view(am, active, m_tile_view=1024, **kw)
    b = R.render_map_view(view, **kw)
    for f in ("images", "tile_indices", "tile_counts"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    img = cpu(a.images)
    assert img.shape == (3, 120, 160, 3)
    assert np.isfinite(img).all() and img.min() >= 0.0 and img.max() <= 1.0 and img.max() > 0.0
    listed = cpu(a.tile_indices)
    assert cpu(view.valid_mask)[listed[listed >= 0]].all() and int(cpu(a.tile_counts).sum()) > 0
    print(f"live map: {n_valid} valid rows, {int((cpu(a.tile_counts) > 0).sum())} tiles hit, image max {img.max():.3f}")
    am.close()


def test_cached_contexts_are_bounded():
    """A sweep over parameters through the functional interface keeps at most MAX_CACHED_RENDERERS contexts:
    the least recently used one is closed."""
    first = R.renderer_for(R.SplatRenderingConfig(max_splats_per_tile=200))
    for cap in range(201, 201 + R.MAX_CACHED_RENDERERS):
        r = R.renderer_for(R.SplatRenderingConfig(max_splats_per_tile=cap))
        assert r.h is not None and len(R._renderers) <= R.MAX_CACHED_RENDERERS
    assert first.h is None and (first.cfg, 0) not in R._renderers
    means = up(np.array([[[5.0, 5.0], [20.0, 9.0]]]))
    Sinv = up(np.broadcast_to(np.eye(2), (1, 2, 2, 2)).copy())
    idx, cnt = R.splat_indices_for_tiles(means, Sinv, 32, 32, max_splats_per_tile=200)   # a fresh context again
    assert cpu(cnt).tolist() == [[[2]]] and cpu(idx)[0, 0, 0, :3].tolist() == [1, 0, -1]
