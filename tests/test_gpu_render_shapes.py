"""GPU tests of the map renderer's three kernels (csrc/gcs_render.hip) at every tile size, cap, list length
and row edge: the edge fixtures recorded from the reference (tests/golden/render_edges.npz), and larger or
hand-built shapes against tests/render_util.py's numpy restatements (held to the fixtures by
test_render_shapes.py) on the kernel's own record.

Bars, the ones test_gpu_rendering.py has: indices and counts equal; tile images on recorded or restated inputs
at rtol 1e-9, atol 1e-12; end-to-end images at rtol 1e-7, atol 1e-7; the kernel's rows against the host
build of them at rtol 1e-12; the per-row record against the reference's operations at rtol 1e-9; fBm at
1e-13.  Everything called bitwise is torch.equal / np.array_equal.

Hand-built lists run at tile 1, 5, 8, 31, 32 with cap 1, 64, 129, 1024, except tile 1 with cap 1024: the numpy
restatement of its 1,920 one-pixel tiles with lists of up to 1,024 rows takes about six seconds, and tile 1
with cap 129 walks the same code with the same list lengths."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import render_util as RU
from gcslam import rendering as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
cpu = lambda x: x.detach().cpu().numpy()  # noqa: E731
up = lambda a: torch.tensor(np.asarray(a), device=DEV)  # noqa: E731
TILE_CASES = tuple(c for c in RU.EDGE_CASES if c != "lattice")      # the lattice case records indices only
W_BIN, H_BIN = 70, 40                                                 # 3 x 2 tiles at tile 32, partial on both edges


def _inputs(sc):
    return (sc["positions"], sc["covariances"], sc["directions"], sc["kappas"], sc["colors"], sc["valid_mask"])


# ---------------------------------------------------------------------- the recorded edges
@pytest.mark.parametrize("name", RU.EDGE_CASES)
def test_prepare_kernel_on_the_edges(name):
    case = RU.load_case(name)
    cfg = RU.splat_config(case)
    kw = dict(fbm_modulate_scale=case["fbm_modulate_scale"], fbm_seed=case["fbm_seed"])
    views = (case["P_pix"], case["offsets"], case["view_dirs"])
    got = {k: cpu(v) for k, v in R.renderer_for(cfg).prepare(*_inputs(case), *views, **kw).items()}
    RU.assert_record(got, case)
    host = R.prepare_splats_host(*_inputs(case), *views, cfg=cfg, **kw)
    for k in ("means", "Sigmas_inv", "alphas", "colors"):
        np.testing.assert_allclose(got[k], host[k], rtol=1e-12, atol=1e-300, err_msg=k)
    assert np.array_equal(got["radii"] == -np.inf, host["radii"] == -np.inf)
    if name == "hard":       # the thin rows mid-sigmoid (test_render_shapes.py holds the host build's to the exact log det)
        import dataclasses
        mid = dataclasses.replace(cfg, logdet0=-37.0)
        thin = (case["family"] == case["family_names"].index("thin")) & case["valid_mask"]
        got = cpu(R.renderer_for(mid).prepare(*_inputs(case), *views)["alphas"])
        host = R.prepare_splats_host(*_inputs(case), *views, cfg=mid)["alphas"]
        assert got[thin].min() < 0.3 and got[thin].max() > 0.6
        np.testing.assert_allclose(got, host, rtol=1e-12, atol=0)


@pytest.mark.parametrize("name", RU.EDGE_CASES)
def test_bin_kernel_on_the_recorded_edges(name):
    """The reference's own call: the valid rows' means and Sigma^-1 in order; indices count those rows.  In the
    lattice case the cap falls inside a group of exact ties: the row decides."""
    case = RU.load_case(name)
    cfg = RU.splat_config(case)
    rows = np.flatnonzero(case["valid_mask"])
    idx, cnt = R.splat_indices_for_tiles(up(case["means"][:, rows]), up(case["Sigmas_inv"][:, rows]), case["width"],
                                         case["height"], cfg.tile_size, cfg.max_splats_per_tile, cfg.eps)
    idx, cnt = cpu(idx), cpu(cnt)
    got = np.where(idx >= 0, rows[np.maximum(idx, 0)], -1)
    assert np.array_equal(cnt, case["tile_counts"])
    assert np.array_equal(got, case["tile_indices"])


@pytest.mark.parametrize("name", TILE_CASES)
def test_render_kernel_on_the_recorded_edges(name):
    case = RU.load_case(name)
    cfg = RU.splat_config(case)
    tiles = R.render_tiles_ewa(up(case["means"]), up(case["Sigmas_inv"]), up(case["alphas"]), up(case["shaded"]),
                               up(case["tile_indices"]), up(case["tile_counts"]), case["width"], case["height"],
                               cfg.tile_size, cfg.ewa_log_clip)
    assert tuple(tiles.shape) == case["tiles"].shape
    np.testing.assert_allclose(cpu(tiles), case["tiles"], rtol=1e-9, atol=1e-12)


def _end_to_end(case, cfg):
    return R.render_map_view(RU.device_view(case), bev=RU.bev_config(case), cfg=cfg, width=case["width"],
                             height=case["height"], pixels_per_metre=case["pixels_per_metre"], centre_xy=case["centre_xy"],
                             fbm_modulate_scale=case["fbm_modulate_scale"], fbm_seed=case["fbm_seed"])


@pytest.mark.parametrize("name", RU.EDGE_CASES)
def test_render_map_view_end_to_end_on_the_edges(name):
    case = RU.load_case(name)
    W, H = case["width"], case["height"]
    res = _end_to_end(case, RU.splat_config(case))
    idx, cnt, img = cpu(res.tile_indices), cpu(res.tile_counts), cpu(res.images)
    assert np.array_equal(cnt, case["tile_counts"]) and np.array_equal(idx, case["tile_indices"])
    assert img.shape == (case["n_views"], H, W, 3) and img.any()
    if case["tiles"] is not None:
        np.testing.assert_allclose(img, RU.image_from_tiles(case["tiles"], W, H), rtol=1e-7, atol=1e-7)


@pytest.mark.parametrize("asked, clamped", [(40, 32), (0, 1)])
def test_tile_size_is_clamped(asked, clamped):
    """tile_size outside [1, 32] is the nearest end of it, bitwise."""
    import dataclasses
    case = RU.load_case("tile5")
    cfg = RU.splat_config(case)
    a = _end_to_end(case, dataclasses.replace(cfg, tile_size=asked))
    b = _end_to_end(case, dataclasses.replace(cfg, tile_size=clamped))
    for f in ("images", "tile_indices", "tile_counts"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    assert a.images.any()


# ---------------------------------------------------------------------- k_rn_render on hand-built lists
W_RN, H_RN, N_RN = 40, 24, 1100


def _render(cfg, rec, alphas, idx, cnt, image_layout=False, colors=None):
    return cpu(R.renderer_for(cfg).render_tiles(up(rec["means"]), up(rec["Sigmas_inv"]), up(alphas),
                                                up(rec["colors"] if colors is None else colors), up(idx), up(cnt), W_RN, H_RN,
                                                image_layout=image_layout))


@pytest.mark.parametrize("tile, cap", [(t, c) for t in (1, 5, 8, 31, 32) for c in (1, 64, 129, 1024) if (t, c) != (1, 1024)])
def test_render_kernel_on_hand_built_lists(tile, cap):
    """List lengths 0, 1, 63, 64, 65, 127, 128, 129 and the cap around the 64-record LDS stage, on tiles that are
    partial on both edges; alphas (N,) and per-view alphas (V, N) that differ between the views; the image
    layout against the tile layout."""
    rng = np.random.default_rng(100 * tile + cap)
    V = 2
    rec = RU.separated_rows(rng, N_RN, W_RN, H_RN, V)
    rec["alphas_vn"][0] = rec["alphas"]
    t, n_ty, n_tx = R.tile_grid(W_RN, H_RN, tile)
    cfg = R.SplatRenderingConfig(tile_size=tile, max_splats_per_tile=cap)
    n_tiles, lengths = V * n_ty * n_tx, set()
    for start in (range(0, 9, n_tiles) if n_tiles < 9 else (0,)):
        idx, cnt = RU.hand_lists(rng, V, n_ty, n_tx, cap, N_RN, start=start)
        lengths |= set(cnt.ravel().tolist())
        ref = RU.render_tiles_np(rec["means"], rec["Sigmas_inv"], rec["alphas_vn"], rec["colors"], idx, cnt, W_RN, H_RN,
                                 tile, cfg.ewa_log_clip)
        per_view = _render(cfg, rec, rec["alphas_vn"], idx, cnt)
        assert per_view.shape == ref.shape == (V, n_ty, n_tx, t, t, 3)
        np.testing.assert_allclose(per_view, ref, rtol=1e-9, atol=1e-12)
        shared = _render(cfg, rec, rec["alphas"], idx, cnt)
        assert np.array_equal(shared[0], per_view[0])
        assert np.array_equal(shared, _render(cfg, rec, np.broadcast_to(rec["alphas"], (V, N_RN)).copy(), idx, cnt))
        if cap > 1:                       # alone in its list a row's alpha cancels in the normalisation
            assert not np.array_equal(shared[1], per_view[1])
        for al in (rec["alphas"], rec["alphas_vn"]):
            img = _render(cfg, rec, al, idx, cnt, image_layout=True)
            assert np.array_equal(img, RU.image_from_tiles(_render(cfg, rec, al, idx, cnt), W_RN, H_RN))
    assert lengths == {min(m, cap) for m in (0, 1, 63, 64, 65, 127, 128, 129, cap)}


def _one_tile_lists(rng, cap, n, length):
    idx = np.full((1, 2, 3, cap), -1, np.int32)
    cnt = np.full((1, 2, 3), length, np.int32)
    for t in np.ndindex(1, 2, 3):
        idx[t][:length] = rng.permutation(n)[:length]
    return idx, cnt


def test_render_kernel_ignores_out_of_range_entries():
    """-1, N and N + 5 inside the counted part weigh nothing: bitwise the list without them (a zero weight adds
    exactly +0).  The holes sit in both LDS stages of a 100-entry list."""
    rng = np.random.default_rng(51)
    cfg = R.SplatRenderingConfig(tile_size=16, max_splats_per_tile=129)
    rec = RU.separated_rows(rng, N_RN, W_RN, H_RN, 1)
    clean, cnt = _one_tile_lists(rng, 129, N_RN, 95)
    holes = {0: -1, 5: N_RN, 63: N_RN + 5, 64: -1, 99: N_RN}
    holed = np.full_like(clean, -1)
    for t in np.ndindex(1, 2, 3):
        rows = iter(clean[t][:95])
        holed[t][:100] = [holes[i] if i in holes else next(rows) for i in range(100)]
    got = _render(cfg, rec, rec["alphas"], holed, np.full_like(cnt, 100))
    assert np.array_equal(got, _render(cfg, rec, rec["alphas"], clean, cnt)) and got.any()


def test_render_kernel_clamps_the_counts():
    """A count above the cap is the cap, a negative count is 0, bitwise."""
    rng = np.random.default_rng(52)
    cfg = R.SplatRenderingConfig(tile_size=16, max_splats_per_tile=65)
    rec = RU.separated_rows(rng, N_RN, W_RN, H_RN, 1)
    idx, cnt = _one_tile_lists(rng, 65, N_RN, 65)
    over, under, zero = cnt.copy(), cnt.copy(), cnt.copy()
    over[0, 0, :] = (66, 1000, 2 ** 31 - 1)
    under[0, 1, :] = zero[0, 1, :] = 0
    under[0, 1, :] = (-1, -65, -2 ** 31)
    full = _render(cfg, rec, rec["alphas"], idx, cnt)
    assert np.array_equal(_render(cfg, rec, rec["alphas"], idx, over), full)
    got = _render(cfg, rec, rec["alphas"], idx, under)
    assert np.array_equal(got, _render(cfg, rec, rec["alphas"], idx, zero))
    assert not got[0, 1].any() and got[0, 0].any()


def test_render_kernel_with_log_clip_zero():
    """ewa_log_clip = 0: every listed row weighs its alpha at every pixel."""
    rng = np.random.default_rng(53)
    cfg = R.SplatRenderingConfig(tile_size=16, max_splats_per_tile=64, ewa_log_clip=0.0)
    rec = RU.separated_rows(rng, N_RN, W_RN, H_RN, 1)
    idx, cnt = _one_tile_lists(rng, 64, N_RN, 40)
    got = _render(cfg, rec, rec["alphas"], idx, cnt)
    ref = RU.render_tiles_np(rec["means"], rec["Sigmas_inv"], rec["alphas"], rec["colors"], idx, cnt, W_RN, H_RN, 16, 0.0)
    np.testing.assert_allclose(got, ref, rtol=1e-9, atol=1e-12)
    for t in np.ndindex(1, 2, 3):
        al, c = rec["alphas"][idx[t][:40]], rec["colors"][0, idx[t][:40]]
        flat = (al[:, None] * c).sum(0) / (al.sum() + 1e-12)
        np.testing.assert_allclose(got[t], np.broadcast_to(flat, (16, 16, 3)), rtol=1e-9, atol=1e-12)


def test_render_kernel_leaves_an_underflowing_pixel_undivided():
    """One tile whose only rows are far and tight: every weight is below 1e-28, so the weight sum + 1e-12 is
    not above 1e-12 and the pixel keeps its undivided colour sum (rendering.py:351-354).  Compared where the
    expected value is a normal number, relative only."""
    rng = np.random.default_rng(54)
    n, tile = 12, 16
    cfg = R.SplatRenderingConfig(tile_size=tile, max_splats_per_tile=64, ewa_log_clip=1.0e4)
    means = np.stack([rng.uniform(24.0, 27.0, n), rng.uniform(24.0, 27.0, n)], 1)[None]      # 12 px or more away
    Sinv = np.broadcast_to(rng.uniform(0.95, 1.2, n)[:, None, None] * np.eye(2), (1, n, 2, 2)).copy()
    rec = dict(means=means, Sigmas_inv=Sinv, colors=rng.uniform(0.2, 1.0, (1, n, 3)))
    alphas = rng.uniform(0.2, 1.0, n)
    idx = np.full((1, 1, 1, 64), -1, np.int32)
    idx[0, 0, 0, :n] = np.arange(n)
    cnt = np.full((1, 1, 1), n, np.int32)
    r = R.renderer_for(cfg)
    got = cpu(r.render_tiles(up(means), up(Sinv), up(alphas), up(rec["colors"]), up(idx), up(cnt), tile, tile))
    ref = RU.render_tiles_np(means, Sinv, alphas, rec["colors"], idx, cnt, tile, tile, tile, 1.0e4)
    py, px = np.meshgrid(np.arange(tile) + 0.5, np.arange(tile) + 0.5, indexing="ij")
    d = np.stack([px, py], -1)[None] - means[0][:, None, None, :]
    ws = (alphas[:, None, None] * np.exp(-0.5 * (d * d).sum(-1) * Sinv[0, :, 0, 0][:, None, None])).sum(0)
    assert ws.max() < 1e-28 and not (ws + 1e-12 > 1e-12).any()             # no pixel is divided
    normal = ref >= np.finfo(np.float64).tiny
    assert normal.mean() > 0.5 and ref.max() < 1e-28
    np.testing.assert_allclose(got[normal], ref[normal], rtol=1e-9, atol=0)
    assert got.max() < 1e-28                                               # divided, it would be 1e12 times that


# ---------------------------------------------------------------------- k_rn_bin at the chunk and sort edges
def _bin(cap, means, radii=None, Sinv=None, cfg_kw=None):
    r = R.renderer_for(R.SplatRenderingConfig(max_splats_per_tile=cap, **(cfg_kw or {})))
    idx, cnt = r.bin_tiles(up(means), None if Sinv is None else up(Sinv), W_BIN, H_BIN,
                           radii=None if radii is None else up(radii))
    return cpu(idx), cpu(cnt)


def _check_bin(cap, means, radii):
    idx, cnt = _bin(cap, means, radii)
    ref_idx, ref_cnt = RU.bin_tiles_np(means, radii, W_BIN, H_BIN, 32, cap)
    assert np.array_equal(cnt, ref_cnt) and np.array_equal(idx, ref_idx)
    return ref_idx, ref_cnt


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 3073, 4096, 4097])
def test_bin_kernel_at_the_chunk_edges(n):
    """Every row overlaps every tile, N around the 1,024-row chunk and the 2,048-entry sort buffer, in ascending,
    descending and random distance order (to tile (0, 0)'s centre), cap 1, 64, 1000 and 1024."""
    for j, order in enumerate(("ascending", "descending", "random")):
        means, radii = RU.ring_scene(np.random.default_rng(10 * n + j), n, order)
        for cap in (1, 64, 1000, 1024):
            _, cnt = _check_bin(cap, means, radii)
            assert (cnt == min(cap, n)).all()


@pytest.mark.parametrize("n, far, keep, per_chunk", [
    (4097, (1,), (), [1024, 0, 1024, 1024, 1]),          # fill 1,024 at the top of the third chunk: no compaction there
    (4097, (1,), (1500,), [1024, 1, 1024, 1024, 1]),     # fill 1,025: one compaction
    (3072, (1,), (), [1024, 0, 1024]),                   # 2,048 entries, never compacted, at the final sort
])
def test_bin_kernel_at_the_fill_edges(n, far, keep, per_chunk):
    """Cap 1024; a chunk's rows are pushed outside so that the fill the kernel looks at is exactly 1,024, 1,025,
    or the whole buffer at the final sort.  Until the first compaction nothing is filtered, so the fill is
    the overlap mask's running count."""
    means, radii = RU.occupancy_scene(np.random.default_rng(61), n, far, keep)
    mask = RU.overlap_mask_np(means, radii, W_BIN, H_BIN, 32)
    for t in np.ndindex(mask.shape[:3]):
        got = [int(c.sum()) for c in np.array_split(mask[t], range(RU.BIN_CHUNK, n, RU.BIN_CHUNK))]
        assert got == per_chunk, (t, got)
    idx, _ = _check_bin(1024, means, radii)
    for i in keep:
        assert (idx[0, 0, 0] == i).any()
    _check_bin(64, means, radii)


@pytest.mark.parametrize("cap", [1, 2, 63, 64, 65, 1023, 1024])
def test_bin_kernel_on_a_lattice_of_ties(cap):
    """4,097 rows on a 0.25 px lattice around tile (0, 0)'s centre: hundreds of groups of exactly equal dist^2,
    and the cap falls inside one: the (dist^2 bits, row) threshold decides which of the tied rows stay."""
    means, radii = RU.lattice_scene(np.random.default_rng(41), 4097)
    assert RU.tiles_tied_at_cap(means[0], W_BIN, H_BIN, 32, cap), "no tile has its cap inside a tie"
    _check_bin(cap, means, radii)


@pytest.mark.parametrize("n", [255, 256, 257, 4097])
def test_bin_kernel_derives_the_radii(n):
    """radii=None (k_rn_radius on the caller's Sigma^-1): bitwise the lists of the radii k_rn_prepare computes
    for the same rows."""
    rng = np.random.default_rng(70 + n)
    V = 3
    sc = RU.random_scene(rng, n, [((20.0, 20.0), n // 4)], 3.0, W_BIN, H_BIN)
    sc["valid_mask"][:] = True
    cfg = R.SplatRenderingConfig(max_splats_per_tile=64)
    s = R.renderer_for(cfg).prepare(*_inputs(sc), *R.view_geometry(R.BEVPushforwardConfig(n_views=V), W_BIN, H_BIN, 1.0,
                                                                   (0.0, 0.0)))
    assert bool(torch.isfinite(s["radii"]).all())
    derived = _bin(64, cpu(s["means"]), Sinv=cpu(s["Sigmas_inv"]))
    given = _bin(64, cpu(s["means"]), radii=cpu(s["radii"]))
    assert np.array_equal(derived[0], given[0]) and np.array_equal(derived[1], given[1])
    ref = RU.bin_tiles_np(cpu(s["means"]), cpu(s["radii"]), W_BIN, H_BIN, 32, 64)
    assert np.array_equal(given[0], ref[0]) and np.array_equal(given[1], ref[1]) and ref[1].max() == min(64, n)


def test_bin_kernel_never_lists_a_dropped_row():
    """A radius of -inf (a dropped row) and a NaN mean (no place in an order) are never listed: the lists are
    those of the scene without these rows."""
    rng = np.random.default_rng(62)
    n = 1500
    means, radii = RU.ring_scene(rng, n, "random")
    bad = np.array([0, 7, 255, 256, 1023, 1024, 1499])
    radii[0, bad[::2]] = -np.inf
    means[0, bad[1::2], 0] = np.nan
    means[0, bad[1], 1] = np.nan
    keep = np.setdiff1d(np.arange(n), bad)
    for cap in (64, 1024):
        idx, cnt = _bin(cap, means, radii)
        ref_idx, ref_cnt = RU.bin_tiles_np(means[:, keep], radii[:, keep], W_BIN, H_BIN, 32, cap)
        assert np.array_equal(cnt, ref_cnt)
        assert np.array_equal(idx, np.where(ref_idx >= 0, keep[np.maximum(ref_idx, 0)], -1))
        assert not np.isin(idx, bad).any()


def test_bin_kernel_with_32_views():
    """GCS_RENDER_MAX_VIEWS views in one call: every view's lists are those of that view run alone."""
    rng = np.random.default_rng(63)
    V, n = 32, 300
    means = np.stack([rng.uniform(0.0, W_BIN, (V, n)), rng.uniform(0.0, H_BIN, (V, n))], -1)
    radii = rng.uniform(0.5, 12.0, (V, n))
    idx, cnt = _bin(16, means, radii)
    ref_idx, ref_cnt = RU.bin_tiles_np(means, radii, W_BIN, H_BIN, 32, 16)
    assert np.array_equal(idx, ref_idx) and np.array_equal(cnt, ref_cnt)
    for v in (0, 1, 17, 31):
        one = _bin(16, means[v:v + 1], radii[v:v + 1])
        assert np.array_equal(one[0][0], idx[v]) and np.array_equal(one[1][0], cnt[v])
    assert len({idx[v].tobytes() for v in range(V)}) == V


# ---------------------------------------------------------------------- k_rn_prepare rows
W_PR, H_PR, PPM_PR = 32, 32, 8.0


def _hard_rows(rng, n):
    """n rows drawn from the hard fixture's valid rows (every family, cond(Sigma') <= 1e6), each at a place of
    its own, with an intensity below 0, inside and above intensity_max."""
    case = RU.load_case("hard")
    rows = np.flatnonzero(case["valid_mask"])
    pick = np.concatenate([rows[[np.flatnonzero(case["family"][rows] == f)[0] for f in range(len(case["family_names"]))]],
                           rng.choice(rows, max(n - len(case["family_names"]), 0))])[:n]
    pick = pick[rng.permutation(pick.shape[0])]
    sc = {k: case[k][pick].copy() for k in RU.INPUTS}
    sc["positions"][:, :2] += rng.uniform(-0.05, 0.05, (n, 2))
    sc["valid_mask"] = rng.uniform(size=n) > 0.1
    sc["valid_mask"][0] = True
    sc["intensity"] = rng.uniform(-50.0, 400.0, n)
    return sc


def _assert_rows(got, want, rtol):
    for k in ("means", "Sigmas_inv", "alphas", "colors"):
        np.testing.assert_allclose(got[k], want[k], rtol=rtol, atol=1e-300 if rtol < 1e-10 else 0, err_msg=k)
    assert np.array_equal(got["radii"] == -np.inf, want["radii"] == -np.inf)
    fin = np.isfinite(want["radii"])
    np.testing.assert_allclose(got["radii"][fin], want["radii"][fin], rtol=max(rtol, 1e-12), atol=0)
    np.testing.assert_allclose(got["fbm"], want["fbm"], rtol=1e-13, atol=0)


@pytest.mark.parametrize("V", [1, 3, 32])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_prepare_kernel_rows(n, V):
    """N around the 256-thread block edge, up to GCS_RENDER_MAX_VIEWS views, rows of every hard family: against
    the host build at rtol 1e-12 and against the reference's operations (prepare_np) at rtol 1e-9, with and
    without intensity, with and without fBm."""
    rng = np.random.default_rng(1000 * V + n)
    sc = _hard_rows(rng, n)
    views = R.view_geometry(R.BEVPushforwardConfig(n_views=V), W_PR, H_PR, PPM_PR, (0.0, 0.0))
    cfg = R.SplatRenderingConfig(tile_size=16, max_splats_per_tile=16, logdet0=-16.0)
    r = R.renderer_for(cfg)
    for intensity, fbm in ((None, 0.0), (sc["intensity"], 0.0), (None, 0.2), (sc["intensity"], 0.2)):
        kw = dict(fbm_modulate_scale=fbm, fbm_seed=5, intensity=intensity)
        got = {k: cpu(v) for k, v in r.prepare(*_inputs(sc), *views, **kw).items()}
        assert got["means"].shape == (V, n, 2) and got["colors"].shape == (V, n, 3)
        host = R.prepare_splats_host(*_inputs(sc), *views, cfg=cfg, **kw)
        _assert_rows(got, host, 1e-12)
        _assert_rows(got, RU.prepare_np(*_inputs(sc), *views, cfg, **kw), 1e-9)
        dropped = ~sc["valid_mask"]
        assert np.all(got["radii"][:, dropped] == -np.inf) and np.isfinite(got["radii"][:, ~dropped]).all()
    if n > 1:
        plain = cpu(r.prepare(*_inputs(sc), *views)["colors"])
        assert not np.array_equal(plain, cpu(r.prepare(*_inputs(sc), *views, intensity=sc["intensity"])["colors"]))


@pytest.mark.parametrize("fbm", [0.0, 0.1])
def test_prepare_kernel_drops_the_rows_it_cannot_process(fbm):
    """A covariance that is not positive definite or is singular, a NaN or infinite position, a NaN kappa,
    direction or colour, an infinite colour under a shading of 0 (inf * 0) and, with fBm on, |x| >= 2^46, on
    rows marked valid, with fBm off and on: each comes out as an invalid row does (radius -inf, zeros, alpha
    and fBm included) and is never listed, and every other row is bitwise what it is with those rows masked
    invalid (the reference would raise or propagate NaN).  With fBm off the rows at
    2^46 are ordinary rows far outside the image."""
    rng = np.random.default_rng(64)
    n, V, W, H = 300, 3, 48, 32
    sc = RU.random_scene(rng, n, [((16.0, 16.0), 60)], 3.0, W, H)
    sc["valid_mask"][:] = True
    bad = dict(not_pd=3, singular=40, zero_cov=41, nan_pos=77, nan_z=78, inf_pos=130, inf_colour=131, nan_dir=200,
               nan_colour=201, nan_kappa=255)
    far = dict(far_x=256, far_y=299)
    sc["covariances"][bad["not_pd"]] = np.diag([1.0, -0.5, 1.0])
    sc["covariances"][bad["singular"]] = np.diag([1.0, 1.0, 0.0])
    sc["covariances"][bad["zero_cov"]] = 0.0
    sc["positions"][bad["nan_pos"], 1] = np.nan
    sc["positions"][bad["nan_z"], 2] = np.nan
    sc["positions"][bad["inf_pos"], 0] = np.inf
    sc["kappas"][bad["nan_kappa"]] = np.nan
    sc["directions"][bad["nan_dir"], 2] = np.nan
    sc["colors"][bad["nan_colour"], 1] = np.nan
    sc["directions"][bad["inf_colour"]] = (0.0, 0.0, 1.0)        # faces up, the views look down: the shading is exactly 0
    sc["kappas"][bad["inf_colour"]] = 1.0e4
    sc["colors"][bad["inf_colour"], 0] = np.inf
    sc["positions"][far["far_x"], 0] = 2.0 ** 46
    sc["positions"][far["far_y"], 1] = -2.0 ** 47
    if fbm > 0.0:
        bad.update(far)
    rows = np.array(sorted(bad.values()))
    masked = dict(sc, valid_mask=~np.isin(np.arange(n), rows))
    cfg = R.SplatRenderingConfig(max_splats_per_tile=32)
    kw = dict(bev=R.BEVPushforwardConfig(n_views=V), cfg=cfg, width=W, height=H, pixels_per_metre=1.0, centre_xy=(0.0, 0.0),
              fbm_modulate_scale=fbm, fbm_seed=3, want_splats=True)
    a = R.render_map_view(RU.device_view(sc), **kw)
    b = R.render_map_view(RU.device_view(masked), **kw)
    s = {k: cpu(v) for k, v in a.splats.items()}
    for name, i in bad.items():
        assert np.all(s["radii"][:, i] == -np.inf), name
        assert not s["means"][:, i].any() and not s["Sigmas_inv"][:, i].any() and not s["colors"][:, i].any(), name
        assert s["alphas"][i] == 0.0 and s["fbm"][i] == 0.0, name
    kept = np.setdiff1d(np.arange(n), rows)
    assert np.isfinite(s["radii"][:, kept]).all() and (s["alphas"][kept] > 0.0).all()
    assert not np.isin(cpu(a.tile_indices), rows).any()
    for k in s:
        assert torch.equal(a.splats[k], b.splats[k]), k
    for f in ("images", "tile_indices", "tile_counts"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    assert bool(torch.isfinite(a.images).all()) and a.images.any()
    host = R.prepare_splats_host(*_inputs(sc), *R.view_geometry(kw["bev"], W, H, 1.0, (0.0, 0.0)), cfg=cfg,
                                 fbm_modulate_scale=fbm, fbm_seed=3)
    assert np.array_equal(host["radii"] == -np.inf, s["radii"] == -np.inf)      # the host build drops the same rows
    assert np.array_equal(host["alphas"] == 0.0, s["alphas"] == 0.0)


def test_prepare_kernel_drops_a_row_in_the_views_that_cannot_shade_it():
    """A row that only some views must drop: its direction is view 0's, kappa 1e6 and one
    colour infinite, so view 0 shades it (inf * s clips to 1) while in views 1 and 2 the shading underflows to 0
    and inf * 0 is NaN.  It keeps its alpha, has view 0's record and radius -inf and zeros in the others, is
    listed by view 0 alone, and views 1 and 2 are bitwise those of the scene with the row masked invalid."""
    rng = np.random.default_rng(68)
    n, V, W, H, row = 200, 3, 48, 32, 17
    sc = RU.random_scene(rng, n, [((16.0, 16.0), 40)], 3.0, W, H)
    sc["valid_mask"][:] = True
    bev = R.BEVPushforwardConfig(n_views=V)
    views = R.view_geometry(bev, W, H, 1.0, (0.0, 0.0))
    sc["positions"][row] = (-8.0, 0.0, 0.1)
    sc["directions"][row] = 2.0 * views[2][0]
    sc["kappas"][row] = 1.0e6
    sc["colors"][row] = (np.inf, 0.5, np.inf)
    masked = dict(sc, valid_mask=np.arange(n) != row)
    kw = dict(bev=bev, cfg=R.SplatRenderingConfig(max_splats_per_tile=200), width=W, height=H, pixels_per_metre=1.0,
              centre_xy=(0.0, 0.0), want_splats=True)
    a = R.render_map_view(RU.device_view(sc), **kw)
    b = R.render_map_view(RU.device_view(masked), **kw)
    s = {k: cpu(v) for k, v in a.splats.items()}
    assert np.isfinite(s["radii"][0, row]) and np.all(s["radii"][1:, row] == -np.inf) and s["alphas"][row] > 0.0
    assert s["colors"][0, row, 0] == 1.0 and 0.0 < s["colors"][0, row, 1] < 1e-5 and s["Sigmas_inv"][0, row].all()
    assert not s["means"][1:, row].any() and not s["Sigmas_inv"][1:, row].any() and not s["colors"][1:, row].any()
    listed = (cpu(a.tile_indices) == row).any((1, 2, 3))
    assert listed.tolist() == [True, False, False]
    for f in ("images", "tile_indices", "tile_counts"):
        assert torch.equal(getattr(a, f)[1:], getattr(b, f)[1:]), f
    assert not torch.equal(a.images[0], b.images[0])
    host = R.prepare_splats_host(*_inputs(sc), *views, cfg=kw["cfg"])
    assert np.array_equal(host["radii"] == -np.inf, s["radii"] == -np.inf) and host["alphas"][row] == s["alphas"][row]


def test_limits_are_refused():
    sc = RU.random_scene(np.random.default_rng(65), 8, [], 1.0, 32, 32)
    with pytest.raises(ValueError):
        R.Renderer(R.SplatRenderingConfig(max_splats_per_tile=1025))
    r = R.renderer_for(R.SplatRenderingConfig())
    with pytest.raises(ValueError):
        r.prepare(*_inputs(sc), *R.view_geometry(R.BEVPushforwardConfig(n_views=33), 32, 32, 1.0, (0.0, 0.0)))
    with pytest.raises(ValueError):
        R.render_map_view(RU.device_view(sc), bev=R.BEVPushforwardConfig(n_views=33), width=32, height=32,
                          pixels_per_metre=1.0, centre_xy=(0.0, 0.0))
    got = r.prepare(*_inputs(sc), *R.view_geometry(R.BEVPushforwardConfig(n_views=32), 32, 32, 1.0, (0.0, 0.0)))
    assert tuple(got["means"].shape) == (32, 8, 2)


# ---------------------------------------------------------------------- gcs_render_view
def _view_call(r, sc, V, W, H, want_splats):
    P_pix, off, vd = R.view_geometry(R.BEVPushforwardConfig(n_views=V), W, H, 1.0, (0.0, 0.0))
    v = RU.device_view(sc)
    return r.render_view(v.positions, v.covariances, v.directions, v.kappas, v.colors, v.valid_mask, P_pix, off, vd, W, H,
                         0.1, 2, want_splats)


def test_render_view_workspace_and_caller_record_agree():
    """want_splats (the caller's record) and the context's workspace: bitwise the same images and lists."""
    sc = RU.random_scene(np.random.default_rng(66), 700, [((20.0, 12.0), 200)], 3.0, 72, 40)
    r = R.Renderer(R.SplatRenderingConfig(max_splats_per_tile=48))
    a, b = _view_call(r, sc, 3, 72, 40, True), _view_call(r, sc, 3, 72, 40, False)
    for f in ("images", "tile_indices", "tile_counts"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    assert a.splats is not None and b.splats is None and a.images.any() and int(a.tile_counts.max()) == 48
    r.close()


def test_render_view_small_call_after_a_large_one():
    """A context whose workspace was grown by N = 5000, V = 3 gives, for N = 10, V = 1, bitwise what a fresh
    context gives (the record's layout inside the workspace depends on the call's N and V alone)."""
    rng = np.random.default_rng(67)
    big = RU.random_scene(rng, 5000, [((30.0, 20.0), 500)], 4.0, 72, 40)
    small = RU.random_scene(rng, 10, [], 1.0, 72, 40)
    small["valid_mask"][:] = True
    cfg = R.SplatRenderingConfig(max_splats_per_tile=16)
    used, fresh = R.Renderer(cfg), R.Renderer(cfg)
    assert _view_call(used, big, 3, 72, 40, False).images.any()
    a, b = _view_call(used, small, 1, 72, 40, False), _view_call(fresh, small, 1, 72, 40, False)
    for f in ("images", "tile_indices", "tile_counts"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    assert a.images.any() and int(a.tile_counts.sum()) >= 10
    used.close()
    fresh.close()
