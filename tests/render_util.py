"""Rendering test helpers (test infrastructure): the fixture loader, a vectorised numpy restatement of the
reference's tile binning (rendering.py:252-289) and tile render (:297-355) for shapes the reference is not
around to run, a numpy restatement of the per-row prepare stage written from the reference's operations
(prepare_np), and the scene builders of the shape tests.  test_rendering_host.py and test_render_shapes.py
hold the restatements to the recorded fixtures (indices exact, tiles at rtol 1e-12, rows at rtol 1e-9)
before any GPU test relies on them."""

import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INPUTS = ("positions", "covariances", "directions", "kappas", "colors", "valid_mask")
STAGE = ("P_pix", "offsets", "view_dirs", "means", "Sigmas_inv", "radii", "alphas", "shaded", "fbm")
TILES = ("tile_indices", "tile_counts", "tiles")
CASES = ("main", "tile8", "cap64", "band", "n1", "n0", "fbm")
EDGE_CASES = ("tile5", "tile1", "tile31", "cfg", "hard", "lattice")     # render_edges.npz; lattice: no tiles recorded
_cache = {}


def _npz(name):
    if name not in _cache:
        _cache[name] = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    return _cache[name]


def load_case(case):
    """One recorded case: the view's row arrays, the call's parameters, the config's fields and every
    stage's recorded output (layout of the view's rows; read-only)."""
    main = _npz("render_main")
    if case in EDGE_CASES:
        src, pre = _npz("render_edges"), case + "_"
        inp, ipre = (main, "") if case == "cfg" else (src, pre)
    elif case == "main":
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
    c.update({k: src[pre + k] for k in STAGE + TILES[:2]})
    c["tiles"] = src.get(pre + "tiles") if case == "lattice" else src[pre + "tiles"]      # lattice: indices only
    p = src[pre + "params"]
    c["phi_center_deg"] = float(p[8]) if p.shape[0] > 8 else 10.0
    if case == "hard":
        c["family"], c["family_names"] = src["hard_family"], tuple(str(f) for f in src["hard_family_names"])
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


def bev_config(case):
    from gcslam.rendering import BEVPushforwardConfig
    return BEVPushforwardConfig(n_views=case["n_views"], phi_center_deg=case["phi_center_deg"])


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
    any fBm factor; weights and colour sums accumulate in list order.  alphas (N,), or (V, N): a view's own."""
    tile = min(max(int(tile), 1), 32)
    alphas = np.asarray(alphas)
    V, n_ty, n_tx = cnt.shape
    out = np.zeros((V, n_ty, n_tx, tile, tile, 3))
    py, px = np.meshgrid(np.arange(tile) + 0.5, np.arange(tile) + 0.5, indexing="ij")
    for v in range(V):
        al = alphas[v] if alphas.ndim == 2 else alphas
        for ty in range(n_ty):
            for tx in range(n_tx):
                acc, ws = np.zeros((tile, tile, 3)), np.zeros((tile, tile))
                for i in idx[v, ty, tx, :cnt[v, ty, tx]]:
                    d0, d1 = (tx * tile + px) - means[v, i, 0], (ty * tile + py) - means[v, i, 1]
                    # d @ Sigma_inv @ d with the first product through numpy's matmul, as the reference has it: on a
                    # Sigma^-1 of cond 1e6 that product cancels, and how it rounds (fused or not: the BLAS build's
                    # choice) shows at 1e-11 in the weight; the plain expression is 7e-12 from the hard fixture
                    t = np.stack([d0, d1], -1) @ Sinv[v, i]
                    q = t[..., 0] * d0 + t[..., 1] * d1
                    w = al[i] * np.exp(np.clip(-0.5 * np.maximum(q, 0.0), -log_clip, 0.0))
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


# ---------------------------------------------------------------------- the prepare stage in numpy
def _hash_float_np(h):
    h = (h * 1103515245 + 12345) & 0x7FFFFFFF
    return h.astype(np.float64) / 2147483648.0


def _value_noise_np(x, y, seed):
    flx, fly = np.floor(x), np.floor(y)
    ix, iy = flx.astype(np.int64), fly.astype(np.int64)
    fx, fy = np.clip(x - flx, 0.0, 1.0), np.clip(y - fly, 0.0, 1.0)
    s31 = np.int64(int(seed) * 31)
    with np.errstate(over="ignore"):       # int64 wrap-around leaves the masked low 31 bits as Python's integers have them
        v00 = _hash_float_np(((s31 + ix) * 31 + iy) & 0x7FFFFFFF)
        v10 = _hash_float_np(((s31 + ix + 1) * 31 + iy) & 0x7FFFFFFF)
        v01 = _hash_float_np(((s31 + ix) * 31 + iy + 1) & 0x7FFFFFFF)
        v11 = _hash_float_np(((s31 + ix + 1) * 31 + iy + 1) & 0x7FFFFFFF)
    sx, sy = fx * fx * (3.0 - 2.0 * fx), fy * fy * (3.0 - 2.0 * fy)
    v0 = v00 * (1 - sx) + v10 * sx
    v1 = v01 * (1 - sx) + v11 * sx
    return v0 * (1 - sy) + v1 * sy


def fbm_np(xy, octaves=5, gain=0.5, seed=0):
    """gcslam.rendering.fbm_at_splat_positions, in numpy."""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    value = np.zeros(xy.shape[0])
    amplitude, frequency, max_amplitude = 1.0, 1.0, 0.0
    for _ in range(int(octaves)):
        value = value + amplitude * _value_noise_np(xy[:, 0] * frequency, xy[:, 1] * frequency, seed)
        max_amplitude += amplitude
        amplitude *= float(gain)
        frequency *= 2.0
    return value / (max_amplitude + 1e-12)


def prepare_np(positions, covariances, directions, kappas, colors, valid_mask, P_pix, offsets, view_dirs, cfg,
               fbm_modulate_scale=0.0, fbm_seed=0, intensity=None):
    """The per-row record of DESIGN.md section 3 from the reference's operations: P mu + b and P Sigma P^T,
    np.linalg.inv, radii_from_inverse, opacity from np.linalg.slogdet, vmf_shading_multi_lobe's formula with
    one lobe (pi = 1, the norms' eps 1e-12, kappa_modulated_by_intensity when an intensity is given), fBm.
    Rows with valid_mask false come out as the kernel writes a dropped row (zeros, radius -inf); which rows
    have to be dropped is the caller's decision, never this function's."""
    pos = np.asarray(positions, np.float64).reshape(-1, 3)
    n = pos.shape[0]
    cov = np.asarray(covariances, np.float64).reshape(n, 3, 3)
    P = np.asarray(P_pix, np.float64).reshape(-1, 2, 3)
    V = P.shape[0]
    off, vd = np.asarray(offsets, np.float64).reshape(V, 2), np.asarray(view_dirs, np.float64).reshape(V, 3)
    rows = np.arange(n) if valid_mask is None else np.flatnonzero(np.asarray(valid_mask).astype(bool))
    out = dict(means=np.zeros((V, n, 2)), Sigmas_inv=np.zeros((V, n, 2, 2)), radii=np.full((V, n), -np.inf),
               alphas=np.zeros(n), colors=np.zeros((V, n, 3)), fbm=np.zeros(n))
    if rows.size == 0:
        return out
    p, S = pos[rows], cov[rows]
    d, k = np.asarray(directions, np.float64).reshape(n, 3)[rows], np.asarray(kappas, np.float64).reshape(n)[rows]
    col = np.asarray(colors, np.float64).reshape(n, 3)[rows]
    with np.errstate(over="ignore"):
        raw = 1.0 / (1.0 + np.exp(-cfg.opacity_gamma * (cfg.logdet0 - np.linalg.slogdet(S)[1])))
    out["alphas"][rows] = cfg.alpha_min + (1.0 - cfg.alpha_min) * raw
    mod = 1.0
    if fbm_modulate_scale > 0.0:
        fb = fbm_np(p[:, :2], cfg.fbm_octaves, cfg.fbm_gain, fbm_seed)
        out["fbm"][rows] = fb
        mod = ((1.0 - fbm_modulate_scale) + fbm_modulate_scale * fb)[:, None]
    mu = d / (np.linalg.norm(d, axis=1, keepdims=True) + 1e-12)
    if cfg.vmf_intensity_scale > 0.0 and intensity is not None and cfg.vmf_intensity_max > 1e-12:
        t = np.asarray(intensity, np.float64).reshape(n)[rows] / max(cfg.vmf_intensity_max, 1e-12)
        k = np.minimum(k * (1.0 + cfg.vmf_intensity_scale * np.clip(t, 0.0, 1.0)), cfg.vmf_kappa_max)
    for v in range(V):
        vn = vd[v] / (np.linalg.norm(vd[v]) + 1e-12)
        S2 = P[v] @ S @ P[v].T
        Sinv = np.linalg.inv(S2)
        s = (0.0 + 1.0 * np.exp(k * (mu @ vn - 1.0))) / (1.0 + k / 1)
        out["means"][v, rows] = p @ P[v].T + off[v]
        out["Sigmas_inv"][v, rows] = Sinv
        out["radii"][v, rows] = radii_from_inverse(Sinv, cfg.eps)
        out["colors"][v, rows] = np.clip(col * s[:, None], 0.0, 1.0) * mod
    return out


# ---------------------------------------------------------------------- scene builders of the shape tests
BIN_CHUNK = 1024          # rows the bin kernel streams between two looks at its fill (kRnChunkRows)


def overlap_mask_np(means, radii, width, height, tile):
    """(V, Ty, Tx, N): bin_tiles_np's overlap test of every row against every tile."""
    tile = min(max(int(tile), 1), 32)
    n_ty, n_tx = -(-height // tile), -(-width // tile)
    mx, my, r = means[:, None, None, :, 0], means[:, None, None, :, 1], np.asarray(radii)[:, None, None, :]
    ox = (np.arange(n_tx) * tile)[None, None, :, None]
    oy = (np.arange(n_ty) * tile)[None, :, None, None]
    return ~((mx + r < ox) | (mx - r > ox + tile) | (my + r < oy) | (my - r > oy + tile))


def ring_scene(rng, n, order, centre=(16.0, 16.0), radius=1.0e3):
    """n rows around `centre` whose radius reaches every tile of a small image, at distinct distances in
    ascending, descending or random row order: (means (1, n, 2), radii (1, n))."""
    d = np.sort(rng.uniform(1.0, 30.0, n))
    d = {"ascending": d, "descending": d[::-1], "random": rng.permutation(d)}[order]
    th = rng.uniform(0.0, 2.0 * np.pi, n)
    means = np.stack([centre[0] + d * np.cos(th), centre[1] + d * np.sin(th)], 1)[None].copy()
    return means, np.full((1, n), radius)


def occupancy_scene(rng, n, far_chunks, keep=()):
    """ring_scene in random order with the rows of the chunks `far_chunks` (0-based, BIN_CHUNK rows each)
    pushed far outside with a small radius, except the rows listed in `keep`, which are moved next to the
    centre instead (they beat any threshold)."""
    means, radii = ring_scene(rng, n, "random")
    for c in far_chunks:
        sl = slice(c * BIN_CHUNK, min((c + 1) * BIN_CHUNK, n))
        means[0, sl] = 1.0e6
        radii[0, sl] = 1.0
    for j, i in enumerate(keep):
        means[0, i] = (16.0 + 0.01 * (j + 1), 16.0)
        radii[0, i] = 1.0e3
    return means, radii


def lattice_scene(rng, n, centre=(16.0, 16.0), half=32, step=0.25, radius=1.0e3):
    """n rows drawn without replacement, in random row order, from the (2 half + 1)^2 points of the `step`
    lattice around `centre`: dist^2 to the centre is exact and shared by 4 or 8 rows where the draw kept
    them, and every row reaches every tile of a small image."""
    g = np.arange(-half, half + 1) * step
    pts = np.stack(np.meshgrid(centre[0] + g, centre[1] + g, indexing="ij"), -1).reshape(-1, 2)
    pts = pts[(pts != np.asarray(centre)).any(1)]        # the centre itself would be a group of one
    assert n <= pts.shape[0]
    means = pts[rng.permutation(pts.shape[0])[:n]][None].copy()
    return means, np.full((1, n), radius)


def sorted_keys(means, centre):
    """A view's dist^2 to `centre`, ascending."""
    return np.sort(((means - np.asarray(centre)) ** 2).sum(-1))


def tiles_tied_at_cap(means, width, height, tile, cap):
    """The (ty, tx) of one view's tiles whose cap-th and (cap + 1)-th keys are equal (every row overlapping)."""
    out = []
    for ty in range(-(-height // tile)):
        for tx in range(-(-width // tile)):
            d2 = sorted_keys(means, ((tx + 0.5) * tile, (ty + 0.5) * tile))
            if cap < d2.shape[0] and d2[cap - 1] == d2[cap]:
                out.append((ty, tx))
    return out


def separated_rows(rng, n, width, height, V=1):
    """A record for the render kernel: n rows on a jittered grid over the image (well separated, no two rows
    alike), random SPD Sigma^-1 with sigma of 1 to 4 px, alphas (N,), per-view alphas (V, N) that differ from
    view to view, colours (V, N, 3)."""
    g = int(np.ceil(np.sqrt(n)))
    cells = rng.permutation(g * g)[:n]
    means = np.stack([(cells % g + rng.uniform(0.2, 0.8, n)) * (width / g), (cells // g + rng.uniform(0.2, 0.8, n)) * (height / g)], 1)
    means = np.broadcast_to(means, (V, n, 2)) + rng.uniform(-0.1, 0.1, (V, n, 2))
    A = rng.normal(size=(V, n, 2, 2))
    Sinv = A @ A.transpose(0, 1, 3, 2) * 0.05 + rng.uniform(0.06, 1.0, (V, n, 1, 1)) * np.eye(2)
    return dict(means=means, Sigmas_inv=Sinv, alphas=rng.uniform(0.05, 1.0, n), alphas_vn=rng.uniform(0.05, 1.0, (V, n)),
                colors=rng.uniform(0.0, 1.0, (V, n, 3)))


def hand_lists(rng, V, n_ty, n_tx, cap, n_rows, lengths=(0, 1, 63, 64, 65, 127, 128, 129, None), start=0):
    """Tile lists built by hand: the tiles' counts cycle through `lengths` from entry `start` on (None: the cap),
    clipped to the cap; every list is a draw of distinct rows in random order, padded with -1."""
    idx = np.full((V, n_ty, n_tx, cap), -1, np.int32)
    cnt = np.zeros((V, n_ty, n_tx), np.int32)
    for j, t in enumerate(np.ndindex(V, n_ty, n_tx)):
        m = lengths[(start + j) % len(lengths)]
        m = min(cap if m is None else m, cap, n_rows)
        idx[t][:m] = rng.permutation(n_rows)[:m]
        cnt[t] = m
    return idx, cnt


def random_scene(rng, n, centres, spread, width, height):
    """n rows on a width x height px image (1 px/m at phi = 0): uniform background plus clusters."""
    pos = np.stack([rng.uniform(-0.5 * width, 0.5 * width, n), rng.uniform(-0.5 * height, 0.5 * height, n),
                    rng.uniform(0.0, 0.5, n)], 1)
    k = 0
    for (cx, cy), m in centres:
        pos[k:k + m, 0] = cx - 0.5 * width + rng.uniform(-spread, spread, m)
        pos[k:k + m, 1] = cy - 0.5 * height + rng.uniform(-spread, spread, m)
        k += m
    A = rng.normal(size=(n, 3, 3)) * np.array([1.2, 1.2, 0.1])
    cov = A @ A.transpose(0, 2, 1) + 0.01 * np.eye(3)
    perm = rng.permutation(n)
    return dict(positions=pos[perm], covariances=cov[perm], directions=rng.normal(size=(n, 3)) + [0.0, -0.2, 1.0],
                kappas=rng.uniform(0.1, 4.0, n), colors=rng.uniform(0.0, 1.0, (n, 3)),
                valid_mask=rng.uniform(size=n) > 0.05)


def check_against_restatement(sc, cfg, V, W, H):
    """render_map_view on a scene: the kernel's rows against the host build of them (rtol 1e-12), then binning
    and the image against the numpy restatements on the kernel's own record.  Returns the counts."""
    from gcslam import rendering as R
    cpu = lambda x: x.detach().cpu().numpy()  # noqa: E731
    res = R.render_map_view(device_view(sc), bev=R.BEVPushforwardConfig(n_views=V), cfg=cfg, width=W, height=H,
                            pixels_per_metre=1.0, centre_xy=(0.0, 0.0), want_splats=True)
    s = {k: cpu(v) for k, v in res.splats.items()}
    P_pix, off, vd = R.view_geometry(R.BEVPushforwardConfig(n_views=V), W, H, 1.0, (0.0, 0.0))
    host = R.prepare_splats_host(sc["positions"], sc["covariances"], sc["directions"], sc["kappas"], sc["colors"],
                                 sc["valid_mask"], P_pix, off, vd, cfg=cfg)
    for k in ("means", "Sigmas_inv", "alphas", "colors"):     # the kernel's rows against the host build of them
        np.testing.assert_allclose(s[k], host[k], rtol=1e-12, atol=1e-300, err_msg=k)
    assert np.array_equal(s["radii"] == -np.inf, host["radii"] == -np.inf)
    # same record in, same decisions out: the comparisons and dist^2 are the same f64 operations
    idx, cnt = bin_tiles_np(s["means"], s["radii"], W, H, cfg.tile_size, cfg.max_splats_per_tile)
    assert np.array_equal(cpu(res.tile_counts), cnt) and np.array_equal(cpu(res.tile_indices), idx)
    tiles = render_tiles_np(s["means"], s["Sigmas_inv"], s["alphas"], s["colors"], idx, cnt, W, H, cfg.tile_size,
                            cfg.ewa_log_clip)
    np.testing.assert_allclose(cpu(res.images), image_from_tiles(tiles, W, H), rtol=1e-9, atol=1e-12)
    return cnt
