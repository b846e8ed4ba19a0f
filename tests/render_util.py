"""Rendering test helpers (test infrastructure): the fixture loader, and a vectorised numpy restatement
of the reference's tile binning (rendering.py:252-289) and tile render (:297-355) for shapes the
reference is not around to run.  test_rendering_host.py holds it to the recorded fixtures (indices
exact, tiles at rtol 1e-12) before any GPU test relies on it."""

import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INPUTS = ("positions", "covariances", "directions", "kappas", "colors", "valid_mask")
STAGE = ("P_pix", "offsets", "view_dirs", "means", "Sigmas_inv", "radii", "alphas", "shaded", "fbm")
TILES = ("tile_indices", "tile_counts", "tiles")
CASES = ("main", "tile8", "cap64", "band", "n1", "n0", "fbm")
_cache = {}


def _npz(name):
    if name not in _cache:
        _cache[name] = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    return _cache[name]


def load_case(case):
    """One recorded case: the view's row arrays, the call's parameters, the config's fields and every
    stage's recorded output (layout of the view's rows; read-only)."""
    main = _npz("render_main")
    if case == "main":
        src, pre, inp, ipre = {**main, **_npz("render_main_tiles")}, "", main, ""
    elif case in ("tile8", "cap64"):
        src, pre, inp, ipre = _npz("render_" + case), "", main, ""
    elif case == "band":
        src, pre, inp, ipre = _npz("render_small"), "band_", main, ""
    elif case in ("n1", "n0"):
        src, pre, inp, ipre = _npz("render_small"), case + "_", _npz("render_small"), case + "_"
    elif case == "fbm":
        src, pre, inp, ipre = _npz("render_fbm"), "", _npz("render_fbm"), ""
    else:
        raise KeyError(case)
    c = {k: inp[ipre + k] for k in INPUTS}
    if case == "band":
        c["valid_mask"] = src["band_valid_mask"]
    c.update({k: src[pre + k] for k in STAGE + TILES})
    p = src[pre + "params"]
    c.update(n_views=int(p[0]), width=int(p[1]), height=int(p[2]), pixels_per_metre=float(p[3]),
             centre_xy=(float(p[4]), float(p[5])), fbm_modulate_scale=float(p[6]), fbm_seed=int(p[7]))
    c["cfg"] = {str(n): float(v) for n, v in zip(src[pre + "cfg_names"], src[pre + "cfg_values"])}
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def splat_config(case):
    from gcslam.rendering import SplatRenderingConfig
    ints = ("tile_size", "max_splats_per_tile", "fbm_octaves")
    return SplatRenderingConfig(**{k: int(v) if k in ints else v for k, v in case["cfg"].items()})


def image_from_tiles(tiles, width, height):
    """(V, Ty, Tx, t, t, 3) -> (V, H, W, 3): the in-image part of every tile."""
    V, n_ty, n_tx, t = tiles.shape[:4]
    return tiles.transpose(0, 1, 3, 2, 4, 5).reshape(V, n_ty * t, n_tx * t, 3)[:, :height, :width]


def radii_from_inverse(Sinv, eps=1e-12):
    """2 / sqrt(max(lambda_min, eps)) with eigvalsh's lower-triangle read, closed form."""
    a, b, c = Sinv[..., 0, 0], Sinv[..., 1, 0], Sinv[..., 1, 1]
    lam = 0.5 * (a + c) - np.sqrt((0.5 * (a - c)) ** 2 + b * b)
    return 2.0 / np.sqrt(np.maximum(lam, eps))


def bin_tiles_np(means, radii, width, height, tile, cap):
    """splat_indices_for_tile over every tile of every view: rows whose [mu +- r] box meets the tile, by
    (dist^2 to the tile centre, row) -- a stable sort on dist^2 of the row-ordered list -- cut at cap."""
    tile = min(max(int(tile), 1), 32)
    V, N = means.shape[:2]
    n_ty, n_tx = -(-height // tile), -(-width // tile)
    idx = np.full((V, n_ty, n_tx, cap), -1, np.int32)
    cnt = np.zeros((V, n_ty, n_tx), np.int32)
    for v in range(V):
        mx, my, r = means[v, :, 0], means[v, :, 1], radii[v]
        for ty in range(n_ty):
            for tx in range(n_tx):
                oy, ox = ty * tile, tx * tile
                out = (mx + r < ox) | (mx - r > ox + tile) | (my + r < oy) | (my - r > oy + tile)
                rows = np.flatnonzero(~out)
                d2 = (mx[rows] - (ox + 0.5 * tile)) ** 2 + (my[rows] - (oy + 0.5 * tile)) ** 2
                keep = rows[np.argsort(d2, kind="stable")][:cap]
                idx[v, ty, tx, :keep.size] = keep
                cnt[v, ty, tx] = keep.size
    return idx, cnt


def render_tiles_np(means, Sinv, alphas, colors, idx, cnt, width, height, tile, log_clip=25.0):
    """render_tile_ewa over every tile of every view: (V, Ty, Tx, t, t, 3).  colors (V, N, 3) already carry
    any fBm factor; weights and colour sums accumulate in list order."""
    tile = min(max(int(tile), 1), 32)
    V, n_ty, n_tx = cnt.shape
    out = np.zeros((V, n_ty, n_tx, tile, tile, 3))
    py, px = np.meshgrid(np.arange(tile) + 0.5, np.arange(tile) + 0.5, indexing="ij")
    for v in range(V):
        for ty in range(n_ty):
            for tx in range(n_tx):
                acc, ws = np.zeros((tile, tile, 3)), np.zeros((tile, tile))
                for i in idx[v, ty, tx, :cnt[v, ty, tx]]:
                    d0, d1 = (tx * tile + px) - means[v, i, 0], (ty * tile + py) - means[v, i, 1]
                    S = Sinv[v, i]
                    q = (d0 * S[0, 0] + d1 * S[1, 0]) * d0 + (d0 * S[0, 1] + d1 * S[1, 1]) * d1
                    w = alphas[i] * np.exp(np.clip(-0.5 * np.maximum(q, 0.0), -log_clip, 0.0))
                    ws += w
                    acc += w[..., None] * colors[v, i]
                total = ws + 1e-12
                acc = np.where((total > 1e-12)[..., None], acc / total[..., None], acc)
                out[v, ty, tx] = np.clip(acc, 0.0, 1.0)
    return out


def assert_record(got, case, rtol=1e-9):
    """The per-row record against the fixture's: mu_px, Sigma^-1, r, alpha and the shaded colours element-wise at
    rtol; fBm at 1e-13; rows that are not valid: radius -inf, the rest zero."""
    valid = case["valid_mask"].astype(bool)
    g = {k: np.asarray(v) for k, v in got.items()}
    np.testing.assert_allclose(g["means"][:, valid], case["means"][:, valid], rtol=rtol, atol=0)
    np.testing.assert_allclose(g["radii"][:, valid], case["radii"][:, valid], rtol=rtol, atol=0)
    np.testing.assert_allclose(g["alphas"][valid], case["alphas"][valid], rtol=rtol, atol=0)
    np.testing.assert_allclose(g["Sigmas_inv"][:, valid], case["Sigmas_inv"][:, valid], rtol=rtol, atol=0)
    s = case["fbm_modulate_scale"]
    mod = ((1.0 - s) + s * case["fbm"])[None, :, None] if s > 0 else 1.0
    np.testing.assert_allclose(g["colors"][:, valid], (case["shaded"] * mod)[:, valid], rtol=rtol, atol=0)
    if s > 0:
        np.testing.assert_allclose(g["fbm"][valid], case["fbm"][valid], rtol=1e-13, atol=0)
    assert np.all(g["radii"][:, ~valid] == -np.inf)
    for k in ("means", "Sigmas_inv", "colors"):
        assert not g[k][:, ~valid].any(), k
    assert not g["alphas"][~valid].any()


def device_view(case, device="cuda:0"):
    """The case's row arrays uploaded into an AtlasMapView (one tile holding every row)."""
    import torch
    from gcslam.association import AtlasMapView
    n = case["kappas"].shape[0]
    up = lambda a, dt=torch.float64: torch.tensor(np.asarray(a), dtype=dt, device=device)  # noqa: E731
    return AtlasMapView(candidate_tile_ids=torch.zeros(n, dtype=torch.int64, device=device),
                        candidate_slots=torch.arange(n, dtype=torch.int32, device=device),
                        valid_mask=up(case["valid_mask"], torch.bool), tile_ids=torch.zeros(1, dtype=torch.int64, device=device),
                        m_tile_view=max(n, 1), positions=up(case["positions"]).reshape(n, 3),
                        directions=up(case["directions"]).reshape(n, 3), kappas=up(case["kappas"]),
                        last_supported_scan_seq=torch.zeros(n, dtype=torch.int64, device=device),
                        covariances=up(case["covariances"]).reshape(n, 3, 3), colors=up(case["colors"]).reshape(n, 3))
