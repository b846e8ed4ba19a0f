#!/usr/bin/env python3
"""Rendering fixtures recorded from the reference's own numpy code (data only).

Runs where a checkout of the reference is present (never on the GPU box).  The two reference files are
pure numpy and are loaded by path (the package __init__ imports jax):
fl_slam_poc/common/bev_pushforward.py and fl_slam_poc/backend/rendering.py.  Every case runs the
reference functions stage by stage -- oblique_Ps_bev15, pushforward_gaussian_3d_to_2d, np.linalg.inv,
opacity_from_logdet(np.linalg.slogdet), vmf_shading_multi_lobe (on copies: it normalises mu_app in
place), fbm_at_splat_positions, splat_indices_for_tile, render_tile_ewa -- in the composition
DESIGN.md section 3 declares, on the valid rows in order, and records each stage in the layout of the
view's rows (an invalid row: zeros, radius -inf).  The tests read only the .npz files.

Main scene (world metres, 8 px/m, 80 x 48 px, tile 32 -> 3 x 2 tiles, partial on both edges, 3 views,
cap 16): ~600 surfel-like rows with thin, randomly oriented covariances, ~10 % invalid (some of them
all zeros); a 40-row cluster in tile (0, 0); two bit-identical rows in it (an exact tie); one row with
its covariance x 400 that overlaps every tile; one row so tight that -q/2 clips at -25 at every pixel;
the right tile column holds a handful of rows (under the cap).  Because the x 400 row reaches every
tile, the empty tiles are in the `band` case (the same scene without that row and without the right
column's rows) and in the N = 1 and N = 0 cases.

Cases: main; tile8 (the scene at 4 px/m on 40 x 24 px, tile 8); cap64 (one view, cap 64); band; n1; n0;
fbm (fbm_modulate_scale 0.15, negative and large world coordinates, 40 x 24 px at tile 16); and
render_ops.npz with the per-element operators (config defaults, projection matrices, eta rotation,
opacity, multi-lobe shading with weights and with intensity modulation on, fBm).

Edge cases (render_edges.npz, a generator of their own, EDGE_SEED; the other files are left as they are):
tile5 (tile 5 on 33 x 21 px, cap 9, 2 views), tile1 (tile 1 on 7 x 5 px, cap 4), tile31 (tile 31 on
63 x 33 px, cap 64), cfg (render_main.npz's rows on 40 x 24 px with opacity_gamma, alpha_min, eps,
ewa_log_clip, logdet0 and tile_size away from their defaults: a radius at the floor and the clip active on
most pixels are asserted), hard (HARD_FAMILIES, each asserted present, cond(Sigma') printed per family and
<= 1e6) and lattice (300 rows on the 0.25 px lattice mirrored about two tile centres, cap 7 inside a group
of exact ties: asserted; indices only).  There an exact dist^2 tie may also be between rows whose means
mirror each other about the tile centre.

The script asserts, and fails otherwise, the conditions that make the fixtures decidable for a second
implementation:
  * each of the four overlap comparisons of every (row, tile, view) has a margin above 1e-6 px;
  * in each tile's sorted dist^2 list consecutive gaps are exactly 0 between bit-identical rows or
    above 1e-6 px^2;
  * the same reference render fed the closed-form 2 x 2 inverse instead of np.linalg.inv differs from
    the recorded image by less than 1e-8 (a tenth of the end-to-end bar);
  * the main scene has a tile over the cap and a tile under it, the band case an empty tile.

Usage: python tests/golden/make_render.py --reference <reference checkout> [--edges-only]
A fixture whose arrays come out as the file on disk has them is not rewritten (a zip member carries its
write time), so an unchanged fixture keeps its bytes.
"""

import argparse
import dataclasses
import importlib.util
import os
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 11
MARGIN = 1e-6
MAX_BYTES = 486243     # the largest fixture committed before these


def load_by_path(root, rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(root, rel))
    mod = importlib.util.module_from_spec(spec)
    import sys
    sys.modules[name] = mod      # dataclasses resolves annotations through sys.modules
    spec.loader.exec_module(mod)
    return mod


def random_rotations(rng, n):
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], 1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], 1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1)], 1)


def surfel_covs(rng, n, s12=(0.05, 0.2), s3=(0.005, 0.02)):
    R = random_rotations(rng, n)
    sig = np.stack([rng.uniform(*s12, n), rng.uniform(*s12, n), rng.uniform(*s3, n)], 1)
    S = np.einsum("nij,nj,nkj->nik", R, sig * sig, R)
    return 0.5 * (S + S.transpose(0, 2, 1))


def make_main_scene(rng):
    """World rows of the main scene; pixel = 8 * world + (40, 24) at phi = 0."""
    px = lambda x, y: ((np.asarray(x) - 40.0) / 8.0, (np.asarray(y) - 24.0) / 8.0)   # noqa: E731
    n_bg = 470
    bx, by = px(rng.uniform(0.5, 58.0, n_bg), rng.uniform(-3.0, 54.0, n_bg))
    pos = [np.stack([bx, by, rng.uniform(0.0, 0.5, n_bg)], 1)]
    cov = [surfel_covs(rng, n_bg)]
    cxs, cys = px(20.0 + rng.uniform(-1.5, 1.5, 40), 12.0 + rng.uniform(-1.5, 1.5, 40))      # the cluster
    cxs[7], cys[7] = px(16.9, 15.2)      # the tied pair's place: among the nearest to tile (0, 0)'s centre
    pos.append(np.stack([cxs, cys, rng.uniform(0.0, 0.2, 40)], 1))
    cov.append(surfel_covs(rng, 40, (0.03, 0.08), (0.004, 0.01)))
    rx, ry = px(rng.uniform(68.0, 78.0, 11), np.r_[rng.uniform(6.0, 26.0, 6), rng.uniform(36.0, 46.0, 5)])
    pos.append(np.stack([rx, ry, rng.uniform(0.0, 0.3, 11)], 1))        # the right tile column
    cov.append(surfel_covs(rng, 11))
    n_free = 76                                                           # rows that will be invalid
    fx, fy = px(rng.uniform(0.0, 80.0, n_free), rng.uniform(0.0, 48.0, n_free))
    pos.append(np.stack([fx, fy, rng.uniform(0.0, 0.5, n_free)], 1))
    cov.append(surfel_covs(rng, n_free))
    pos, cov = np.concatenate(pos), np.concatenate(cov)
    n = pos.shape[0]
    role = np.zeros(n, np.int32)          # 0 background, 1 cluster, 2 right column, 3 invalid, 4.. specials
    role[n_bg:n_bg + 40], role[n_bg + 40:n_bg + 51], role[n_bg + 51:] = 1, 2, 3
    # specials appended: the tie's twin, the x 400 row, the tight row
    twin_of = n_bg + 7
    big_p = np.array([[0.1, -0.05, 0.1]])
    Rz = np.eye(3)
    big_c = (Rz * np.array([0.15, 0.13, 0.01]) ** 2) * 400.0
    big_c[0, 1] = big_c[1, 0] = 0.2 * 400.0 * 0.15 * 0.13 * 0.5
    tx_, ty_ = px(72.3, 15.6)
    tight_p = np.array([[float(tx_), float(ty_), 0.1]])
    tight_c = surfel_covs(rng, 1, (0.0015, 0.0025), (0.0004, 0.0006))
    pos = np.concatenate([pos, pos[twin_of:twin_of + 1], big_p, tight_p])
    cov = np.concatenate([cov, cov[twin_of:twin_of + 1], big_c[None], tight_c])
    role = np.concatenate([role, [4, 5, 6]]).astype(np.int32)
    n = pos.shape[0]
    d = rng.normal(size=(n, 3)) + np.array([0.0, -0.3, 1.0])             # mostly facing the sweep
    d *= rng.uniform(0.5, 2.0, (n, 1))                                    # not unit: the shading normalises
    kappa = rng.uniform(0.5, 20.0, n)
    col = rng.uniform(0.0, 1.0, (n, 3))
    col[::7] *= 6.0                                                       # some shaded colours reach the clip
    tw = n - 3
    d[tw], kappa[tw], col[tw] = d[twin_of], kappa[twin_of], col[twin_of]  # bit-identical rows
    perm = rng.permutation(n)                                             # no structure in the row order
    pos, cov, d, kappa, col, role = pos[perm], cov[perm], d[perm], kappa[perm], col[perm], role[perm]
    valid = role != 3
    zero = np.flatnonzero(~valid)[:5]                                     # empty slots of a view: all zeros
    pos[zero], cov[zero], d[zero], kappa[zero], col[zero] = 0.0, 0.0, 0.0, 0.0, 0.0
    return dict(positions=pos, covariances=cov, directions=d, kappas=kappa, colors=col, valid_mask=valid, role=role)


def closed_form_inv(S):
    det = S[0, 0] * S[1, 1] - S[0, 1] * S[1, 0]
    return np.array([[S[1, 1], -S[0, 1]], [-S[1, 0], S[0, 0]]]) / det


def run_case(rr, rb, scene, *, n_views, width, height, ppm, centre, cfg_kw, fbm_scale=0.0, fbm_seed=0,
             check_closed_form=True, bev_kw=None, mirror_ties=False, with_tiles=True):
    """The declared composition through the reference's functions.  Returns the record of every stage.
    bev_kw (the edge cases): further BEVPushforwardConfig fields; phi_center_deg is then recorded as params[8].
    mirror_ties: an exact dist^2 tie may also be between rows whose means mirror each other about the tile
    centre.  with_tiles=False records the indices only."""
    cfg = rr.SplatRenderingConfig(**cfg_kw)
    bev = rb.BEVPushforwardConfig(n_views=n_views, **(bev_kw or {}))
    Ps = rb.oblique_Ps_bev15(bev)
    V = Ps.shape[0]
    phis_deg = (np.array([bev.phi_center_deg]) if V == 1 else
                bev.phi_center_deg + np.linspace(-0.5, 0.5, V, dtype=np.float64) * bev.phi_span_deg)
    pos, cov = scene["positions"], scene["covariances"]
    N = pos.shape[0]
    rows = np.flatnonzero(scene["valid_mask"])
    nv = rows.shape[0]
    tile = min(max(int(cfg.tile_size), 1), 32)
    n_ty, n_tx = -(-height // tile), -(-width // tile)
    cap = cfg.max_splats_per_tile
    out = dict(P_pix=np.zeros((V, 2, 3)), offsets=np.zeros((V, 2)), view_dirs=np.zeros((V, 3)),
               means=np.zeros((V, N, 2)), Sigmas_inv=np.zeros((V, N, 2, 2)), radii=np.full((V, N), -np.inf),
               alphas=np.zeros(N), shaded=np.zeros((V, N, 3)), fbm=np.zeros(N),
               tile_indices=np.full((V, n_ty, n_tx, cap), -1, np.int32), tile_counts=np.zeros((V, n_ty, n_tx), np.int32),
               tiles=np.zeros((V, n_ty, n_tx, tile, tile, 3)), images=np.zeros((V, height, width, 3)))
    for i in rows:
        out["alphas"][i] = rr.opacity_from_logdet(np.linalg.slogdet(cov[i])[1], cfg.opacity_gamma, cfg.logdet0,
                                                  cfg.alpha_min)
    if nv:
        out["fbm"][rows] = rr.fbm_at_splat_positions(pos[rows, :2], octaves=cfg.fbm_octaves, gain=cfg.fbm_gain,
                                                     seed=fbm_seed)
    min_margin, max_cf = np.inf, 0.0
    for k in range(V):
        P_pix = ppm * Ps[k]
        b = np.array([0.5 * width, 0.5 * height]) - P_pix @ np.array([centre[0], centre[1], 0.0])
        phi = np.deg2rad(phis_deg[k])
        v = np.array([0.0, np.sin(phi), -np.cos(phi)])
        out["P_pix"][k], out["offsets"][k], out["view_dirs"][k] = P_pix, b, v
        means, Sinv, Sinv_cf, shaded = np.zeros((nv, 2)), np.zeros((nv, 2, 2)), np.zeros((nv, 2, 2)), np.zeros((nv, 3))
        for j, i in enumerate(rows):
            mu2, S2 = rb.pushforward_gaussian_3d_to_2d(pos[i], cov[i], P_pix)
            means[j], Sinv[j], Sinv_cf[j] = mu2 + b, np.linalg.inv(S2), closed_form_inv(S2)
            s = rr.vmf_shading_multi_lobe(v, scene["directions"][i:i + 1].copy(), scene["kappas"][i:i + 1].copy())
            shaded[j] = np.clip(scene["colors"][i] * s, 0.0, 1.0)
        out["means"][k, rows], out["Sigmas_inv"][k, rows], out["shaded"][k, rows] = means, Sinv, shaded
        radii = np.array([2.0 / np.sqrt(max(float(np.min(np.linalg.eigvalsh(Sinv[j]))), cfg.eps)) for j in range(nv)])
        out["radii"][k, rows] = radii
        alphas = out["alphas"][rows]
        world = pos[rows, :2]
        for ty in range(n_ty):
            for tx in range(n_tx):
                oy, ox = ty * tile, tx * tile
                if nv:
                    mx, my = means[:, 0], means[:, 1]
                    m4 = np.stack([mx + radii - ox, mx - radii - (ox + tile), my + radii - oy, my - radii - (oy + tile)])
                    min_margin = min(min_margin, float(np.min(np.abs(m4))))
                    over = ~((m4[0] < 0) | (m4[1] > 0) | (m4[2] < 0) | (m4[3] > 0))
                    d2 = np.sort(((mx - (ox + 0.5 * tile)) ** 2 + (my - (oy + 0.5 * tile)) ** 2)[over])
                    gaps = np.diff(d2)
                    assert np.all((gaps == 0.0) | (gaps > MARGIN)), ("dist^2 gap", k, ty, tx, gaps[gaps <= MARGIN])
                    for g in np.flatnonzero(gaps == 0.0):      # an exact tie is between bit-identical rows only
                        tied = np.flatnonzero(over & (((mx - (ox + 0.5 * tile)) ** 2 +
                                                        (my - (oy + 0.5 * tile)) ** 2) == d2[g]))
                        c = np.array([ox + 0.5 * tile, oy + 0.5 * tile])
                        first = means[tied[0]]
                        assert all(np.array_equal(means[t], first) or
                                   (mirror_ties and np.array_equal(np.sort(np.abs(means[t] - c)), np.sort(np.abs(first - c))))
                                   for t in tied), ("tie", k, ty, tx, tied)
                idx = rr.splat_indices_for_tile((oy, ox), tile, means, Sinv, cap, cfg.eps)
                out["tile_indices"][k, ty, tx, :idx.size] = rows[idx]
                out["tile_counts"][k, ty, tx] = idx.size
                if not with_tiles:
                    continue
                kw = dict(splat_indices=idx, log_clip=cfg.ewa_log_clip, means_world_xy=world,
                          fbm_octaves=cfg.fbm_octaves, fbm_gain=cfg.fbm_gain, fbm_seed=fbm_seed,
                          fbm_modulate_scale=fbm_scale)
                t = rr.render_tile_ewa((oy, ox), tile, means, Sinv, alphas, shaded, **kw)
                out["tiles"][k, ty, tx] = t
                h, w = min(tile, height - oy), min(tile, width - ox)
                out["images"][k, oy:oy + h, ox:ox + w] = t[:h, :w]
                if check_closed_form and nv:
                    t2 = rr.render_tile_ewa((oy, ox), tile, means, Sinv_cf, alphas, shaded, **kw)
                    max_cf = max(max_cf, float(np.max(np.abs(t2 - t))))
    assert min_margin > MARGIN, f"overlap margin {min_margin}"
    assert max_cf < 1e-8, f"closed-form inverse moves the image by {max_cf}"
    out["params"] = np.array([n_views, width, height, ppm, centre[0], centre[1], fbm_scale, fbm_seed] +
                             ([bev.phi_center_deg] if bev_kw is not None else []), np.float64)
    out["cfg_names"] = np.array([f.name for f in dataclasses.fields(cfg)])
    out["cfg_values"] = np.array([float(getattr(cfg, f.name)) for f in dataclasses.fields(cfg)])
    stats = dict(min_margin=min_margin, closed_form_diff=max_cf,
                 cond=float(max((np.linalg.cond(np.linalg.inv(out["Sigmas_inv"][k, i])) for k in range(V) for i in rows),
                                default=0.0)),
                 alpha=(float(out["alphas"][rows].min()), float(out["alphas"][rows].max())) if nv else (0.0, 0.0))
    return out, stats


def ops_fixture(rr, rb, rng):
    o = {}
    for name, cls in (("splat", rr.SplatRenderingConfig), ("bev", rb.BEVPushforwardConfig)):
        c = cls()
        o[f"{name}_names"] = np.array([f.name for f in dataclasses.fields(c)])
        o[f"{name}_defaults"] = np.array([float(getattr(c, f.name)) for f in dataclasses.fields(c)])
    o["Ps_default"] = rb.oblique_Ps_bev15(rb.BEVPushforwardConfig())
    o["Ps_cfg"] = np.array([4.0, 22.5, 31.0])                      # n_views, phi_center_deg, phi_span_deg
    o["Ps_custom"] = rb.oblique_Ps_bev15(rb.BEVPushforwardConfig(n_views=4, phi_center_deg=22.5, phi_span_deg=31.0))
    o["Ps_one"] = rb.oblique_Ps_bev15(rb.BEVPushforwardConfig(n_views=1, phi_center_deg=33.0))
    n = 64
    R = random_rotations(rng, 1)[0]
    etas = rng.normal(size=(n, 3)) * rng.uniform(0.1, 30.0, (n, 1))
    o["rot_R"], o["rot_etas"], o["rot_out"] = R, etas, rb.rotate_vmf_etas(R, etas)
    mu, S = rng.normal(size=(n, 3)) * 5.0, surfel_covs(rng, n)
    P = o["Ps_custom"] * 6.5
    o["pf_mu"], o["pf_Sigma"], o["pf_P"] = mu, S, P
    o["pf_mu2"] = np.array([[rb.pushforward_gaussian_3d_to_2d(mu[i], S[i], P[k])[0] for i in range(n)] for k in range(4)])
    o["pf_S2"] = np.array([[rb.pushforward_gaussian_3d_to_2d(mu[i], S[i], P[k])[1] for i in range(n)] for k in range(4)])
    ld = rng.uniform(-30.0, 30.0, n)
    o["op_logdet"] = ld
    o["op_args"] = np.array([0.7, -3.0, 0.05])
    o["op_default"] = np.array([rr.opacity_from_logdet(x) for x in ld])
    o["op_custom"] = np.array([rr.opacity_from_logdet(x, 0.7, -3.0, 0.05) for x in ld])
    B = 3
    lobes = rng.normal(size=(n, B, 3)) * rng.uniform(0.2, 3.0, (n, B, 1))
    kap = rng.uniform(0.0, 80.0, (n, B))
    pi = rng.uniform(0.1, 1.0, B)
    inten = rng.uniform(-20.0, 300.0, (n, B))                      # below 0 and above intensity_max: clamped
    v = np.array([0.3, 0.5, -0.8])
    o["vmf_v"], o["vmf_mu"], o["vmf_kappa"], o["vmf_pi"], o["vmf_intensity"] = v, lobes, kap, pi, inten
    o["vmf_plain"] = np.array([rr.vmf_shading_multi_lobe(v.copy(), lobes[i].copy(), kap[i].copy()) for i in range(n)])
    o["vmf_pi_out"] = np.array([rr.vmf_shading_multi_lobe(v.copy(), lobes[i].copy(), kap[i].copy(), pi_b=pi.copy())
                                for i in range(n)])
    o["vmf_int_args"] = np.array([0.5, 255.0, 100.0])              # intensity_scale, intensity_max, kappa_max
    o["vmf_int_out"] = np.array([rr.vmf_shading_multi_lobe(v.copy(), lobes[i].copy(), kap[i].copy(), pi_b=pi.copy(),
                                                           intensity=inten[i].copy(), intensity_scale=0.5,
                                                           intensity_max=255.0, kappa_max=100.0) for i in range(n)])
    # one lobe per row with intensity, as gcs_render_prepare shades
    o["vmf1_intensity"] = inten[:, 0].copy()
    o["vmf1_out"] = np.array([rr.vmf_shading_multi_lobe(v.copy(), lobes[i, :1].copy(), kap[i, :1].copy(),
                                                        intensity=inten[i, :1].copy(), intensity_scale=0.5,
                                                        intensity_max=255.0, kappa_max=100.0) for i in range(n)])
    xy = np.concatenate([rng.uniform(-50.0, 50.0, (n, 2)), rng.uniform(-3e6, 3e6, (n, 2)),
                         np.array([[0.0, 0.0], [-1.0, -1.0], [-0.5, 7.0], [123456789.25, -987654321.5]])])
    o["fbm_xy"] = xy
    o["fbm_default"] = rr.fbm_at_splat_positions(xy)
    o["fbm_args"] = np.array([7.0, 0.6, 12345.0])                  # octaves, gain, seed
    o["fbm_custom"] = rr.fbm_at_splat_positions(xy, octaves=7, gain=0.6, seed=12345)
    return o


def save(name, arrays):
    path = os.path.join(HERE, name)
    if os.path.exists(path):      # a zip member carries its write time: an unchanged fixture keeps its bytes
        with np.load(path) as old:
            if sorted(old.files) == sorted(arrays) and all(
                    np.asarray(arrays[k]).dtype == old[k].dtype and
                    np.array_equal(old[k], arrays[k], equal_nan=np.asarray(arrays[k]).dtype.kind == "f")
                    for k in arrays):
                print(f"  {name}: unchanged")
                return
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, f"{name}: {size} bytes"
    print(f"  wrote {name}: {size / 1024:.0f} KB")


STAGE = ("P_pix", "offsets", "view_dirs", "means", "Sigmas_inv", "radii", "alphas", "shaded", "fbm", "params",
         "cfg_names", "cfg_values")
TILES = ("tile_indices", "tile_counts", "tiles")
INPUTS = ("positions", "covariances", "directions", "kappas", "colors", "valid_mask")


# ---------------------------------------------------------------------- the edge cases (render_edges.npz)
EDGE_SEED = 23
HARD_FAMILIES = ("surfel", "thin", "needle", "huge", "tiny", "kappa0", "kappa1e4", "antiparallel", "zero_dir",
                 "colour_range", "ulp_asym")


def small_scene(rng, n, width, height, ppm, n_cluster=0, cluster_px=(0.0, 0.0), cluster_spread=1.0, s12=(0.05, 0.2),
                s3=(0.005, 0.02)):
    """n surfel-like rows over a width x height px image centred on the world origin, the first n_cluster of
    them around one pixel; about 8 % invalid; row order shuffled."""
    ux, uy = rng.uniform(-1.0, width + 1.0, n), rng.uniform(-1.0, height + 1.0, n)
    ux[:n_cluster] = cluster_px[0] + rng.uniform(-cluster_spread, cluster_spread, n_cluster)
    uy[:n_cluster] = cluster_px[1] + rng.uniform(-cluster_spread, cluster_spread, n_cluster)
    pos = np.stack([(ux - 0.5 * width) / ppm, (uy - 0.5 * height) / ppm, rng.uniform(0.0, 0.3, n)], 1)
    d = rng.normal(size=(n, 3)) + np.array([0.0, -0.3, 1.0])
    sc = dict(positions=pos, covariances=surfel_covs(rng, n, s12, s3), directions=d * rng.uniform(0.5, 2.0, (n, 1)),
              kappas=rng.uniform(0.5, 20.0, n), colors=rng.uniform(0.0, 1.0, (n, 3)), valid_mask=rng.uniform(size=n) > 0.08)
    perm = rng.permutation(n)
    return {k: v[perm] for k, v in sc.items()}


def rotated_covs(rng, sig):
    R = random_rotations(rng, sig.shape[0])
    S = np.einsum("nij,nj,nkj->nik", R, sig * sig, R)
    return 0.5 * (S + S.transpose(0, 2, 1))


def view_dirs_of(rb, n_views):
    bev = rb.BEVPushforwardConfig(n_views=n_views)
    phis = np.deg2rad(bev.phi_center_deg + np.linspace(-0.5, 0.5, n_views) * bev.phi_span_deg)
    return np.stack([np.zeros(n_views), np.sin(phis), -np.cos(phis)], 1)


def conds_of(rb, cov, Ps):
    """cond(Sigma') of every (view, row)."""
    return np.array([[np.linalg.cond(rb.pushforward_gaussian_3d_to_2d(np.zeros(3), c, P)[1]) for c in cov] for P in Ps])


def make_hard_scene(rng, rb, n_views, width, height, ppm):
    """The row families of the `hard` case (HARD_FAMILIES), cond(Sigma') <= 1e6 in every view."""
    Ps = ppm * rb.oblique_Ps_bev15(rb.BEVPushforwardConfig(n_views=n_views))
    vd = view_dirs_of(rb, n_views)
    counts = dict(surfel=70, thin=24, needle=16, huge=6, tiny=8, kappa0=6, kappa1e4=6, antiparallel=6, zero_dir=4,
                  colour_range=12, ulp_asym=4)
    fam, cov = [], []
    for f, name in enumerate(HARD_FAMILIES):
        m = counts[name]
        fam += [f] * m
        if name == "thin":
            got = []
            while len(got) < m:       # sigma_3 about 1e-6; an orientation seen too close to edge-on is drawn again
                c = rotated_covs(rng, np.array([[rng.uniform(0.05, 0.2), rng.uniform(0.05, 0.2), rng.uniform(0.5e-6, 2e-6)]]))
                if conds_of(rb, c, Ps).max() <= 1e6:
                    got.append(c[0])
            cov.append(np.array(got))
        elif name == "needle":
            got = []
            while len(got) < m:       # long axis near the image plane: cond(Sigma') ~ (sigma_1 / sigma_2)^2
                s = rng.uniform(0.3, 0.6)
                ratio = rng.uniform(350.0, 950.0)
                th = rng.uniform(0.0, np.pi)
                ax = np.array([np.cos(th), np.sin(th), rng.uniform(-0.1, 0.1)])
                ax /= np.linalg.norm(ax)
                c = (s / ratio) ** 2 * np.eye(3) + (s * s - (s / ratio) ** 2) * np.outer(ax, ax)
                c = 0.5 * (c + c.T)
                k = conds_of(rb, c[None], Ps)
                if k.min() >= 1e5 and k.max() <= 1e6:
                    got.append(c)
            cov.append(np.array(got))
        elif name == "huge":
            cov.append(rotated_covs(rng, rng.uniform(2e5, 1e6, (m, 3))))
        elif name == "tiny":
            cov.append(rotated_covs(rng, rng.uniform(0.5e-5, 2e-5, (m, 3))))
        else:
            cov.append(surfel_covs(rng, m))
    fam, cov = np.array(fam, np.int32), np.concatenate(cov)
    n = fam.shape[0]
    F = {name: fam == f for f, name in enumerate(HARD_FAMILIES)}
    ux, uy = rng.uniform(1.0, width - 1.0, n), rng.uniform(1.0, height - 1.0, n)
    pos = np.stack([(ux - 0.5 * width) / ppm, (uy - 0.5 * height) / ppm, rng.uniform(0.0, 0.3, n)], 1)
    d = (rng.normal(size=(n, 3)) * 0.3 + np.array([0.0, -0.3, 1.0])) * rng.uniform(0.5, 2.0, (n, 1))
    kappa = rng.uniform(0.5, 20.0, n)
    col = rng.uniform(0.0, 1.0, (n, 3))
    kappa[F["kappa0"]] = 0.0
    kappa[F["kappa1e4"]] = 1.0e4          # directions face up, the views look down: exp(-1e4 (1 - cos)) is 0
    d[F["kappa1e4"], 2] = np.abs(d[F["kappa1e4"], 2]) + 0.5
    for j, i in enumerate(np.flatnonzero(F["antiparallel"])):
        d[i] = -vd[j % n_views] * rng.uniform(0.5, 2.0)
    d[F["zero_dir"]] = 0.0
    col[F["colour_range"]] = rng.uniform(-0.5, 6.0, (int(F["colour_range"].sum()), 3))
    col[np.flatnonzero(F["colour_range"])[0]] = [-0.25, 0.5, 7.0]
    for i in np.flatnonzero(F["ulp_asym"]):        # the upper triangle one ulp away from the lower
        cov[i, 0, 1] = np.nextafter(cov[i, 0, 1], np.inf)
        cov[i, 1, 2] = np.nextafter(cov[i, 1, 2], -np.inf)
    valid = rng.uniform(size=n) > 0.06
    valid[[np.flatnonzero(m)[0] for m in F.values()]] = True       # every family keeps a valid row
    perm = rng.permutation(n)
    return dict(positions=pos[perm], covariances=cov[perm], directions=d[perm], kappas=kappa[perm], colors=col[perm],
                valid_mask=valid[perm], family=fam[perm])


def make_lattice_scene(rng, n_rows=300, width=64, height=32, tile=32, sigma=40.0):
    """Pixel means on the 0.25 lattice, in groups mirrored about a tile centre ((+-a, +-b): 4 rows; with
    (+-b, +-a) too: 8 rows), so that every dist^2 to either centre is shared exactly; no two groups share a
    dist^2.  1 px/m, phi = 0 and the image centred on the world origin: pixel = world + (W/2, H/2), exactly."""
    centres = [(0.5 * tile + tile * tx, 0.5 * tile) for tx in range(width // tile)]
    used = [set() for _ in centres]
    pts = []
    g = 0
    while len(pts) < n_rows:
        a, b = rng.integers(1, 60, 2) * 0.25
        if a == b:
            continue
        offs = [(sx * a, sy * b) for sx in (-1, 1) for sy in (-1, 1)]
        if g % 2 == 0 and len(pts) + 8 <= n_rows:
            offs += [(sx * b, sy * a) for sx in (-1, 1) for sy in (-1, 1)]
        cx, cy = centres[(g // 2) % len(centres)]
        grp = [(cx + dx, cy + dy) for dx, dy in offs]
        d2 = [set((x - c[0]) ** 2 + (y - c[1]) ** 2 for x, y in grp) for c in centres]
        if any(d2[k] & used[k] for k in range(len(centres))):
            continue
        for k in range(len(centres)):
            used[k] |= d2[k]
        pts += grp
        g += 1
    px = np.array(pts)[rng.permutation(n_rows)]
    pos = np.stack([px[:, 0] - 0.5 * width, px[:, 1] - 0.5 * height, np.zeros(n_rows)], 1)
    cov = np.broadcast_to(sigma * sigma * np.eye(3), (n_rows, 3, 3)).copy()
    d = np.broadcast_to(np.array([0.0, 0.0, 1.0]), (n_rows, 3)).copy()      # one look for every row: only the order is recorded
    return dict(positions=pos, covariances=cov, directions=d, kappas=np.ones(n_rows), colors=np.full((n_rows, 3), 0.5),
                valid_mask=np.ones(n_rows, bool))


def clip_fraction(out, k, width, height, log_clip):
    """Per row of view k: the fraction of the image's pixel centres at which -q/2 is clipped at -log_clip."""
    py, px = np.meshgrid(np.arange(height) + 0.5, np.arange(width) + 0.5, indexing="ij")
    d = np.stack([px, py], -1)[None] - out["means"][k][:, None, None, :]
    q = np.einsum("nhwi,nij,nhwj->nhw", d, out["Sigmas_inv"][k], d)
    return (0.5 * np.maximum(q, 0.0) > log_clip).mean((1, 2))


def edge_cases(rr, rb):
    rng = np.random.default_rng(EDGE_SEED)
    edges = {}

    def put(name, scene, out, tiles=True, inputs=True):
        if inputs:
            edges.update({f"{name}_{k}": scene[k] for k in INPUTS})
        edges.update({f"{name}_{k}": out[k] for k in STAGE + (TILES if tiles else TILES[:2])})

    for name, n, kw in (
            ("tile5", 150, dict(n_views=2, width=33, height=21, ppm=4.0, cfg_kw=dict(tile_size=5, max_splats_per_tile=9,
                                                                                     logdet0=-14.0))),
            ("tile1", 60, dict(n_views=1, width=7, height=5, ppm=2.0, cfg_kw=dict(tile_size=1, max_splats_per_tile=4,
                                                                                  logdet0=-12.0))),
            ("tile31", 200, dict(n_views=1, width=63, height=33, ppm=8.0, cfg_kw=dict(tile_size=31, max_splats_per_tile=64,
                                                                                      logdet0=-16.0)))):
        sc = small_scene(rng, n, kw["width"], kw["height"], kw["ppm"], n_cluster=n // 3,
                         cluster_px=(0.3 * kw["width"], 0.4 * kw["height"]), cluster_spread=0.1 * kw["width"])
        out, st = run_case(rr, rb, sc, centre=(0.0, 0.0), bev_kw={}, **kw)
        cnt, cap = out["tile_counts"], kw["cfg_kw"]["max_splats_per_tile"]
        print(f"{name}: {n} rows, min margin {st['min_margin']:.2e} px, closed-form diff {st['closed_form_diff']:.2e}, "
              f"counts {cnt.min()}..{cnt.max()}, tiles at the cap {int((cnt == cap).sum())} of {cnt.size}")
        assert (cnt == cap).any() and (cnt < cap).any(), name
        put(name, sc, out)

    main = dict(np.load(os.path.join(HERE, "render_main.npz")))
    sc = {k: main[k] for k in INPUTS}
    cw, ch = 40, 24          # the tile8 case's geometry; the rows are render_main.npz's and are not stored again
    kw = dict(n_views=1, width=cw, height=ch, ppm=4.0, centre=(0.0, 0.0), bev_kw={},
              cfg_kw=dict(tile_size=16, max_splats_per_tile=16, opacity_gamma=0.7, alpha_min=0.05, eps=1e-2,
                          ewa_log_clip=3.0, logdet0=-12.0))
    out, st = run_case(rr, rb, sc, **kw)
    valid = sc["valid_mask"]
    floor = 2.0 / np.sqrt(kw["cfg_kw"]["eps"])
    at_floor = int((out["radii"][:, valid] == floor).sum())
    listed = np.unique(out["tile_indices"][0][out["tile_indices"][0] >= 0])
    clipped = float(np.mean(clip_fraction(out, 0, cw, ch, 3.0)[listed]))
    print(f"cfg: min margin {st['min_margin']:.2e} px, closed-form diff {st['closed_form_diff']:.2e}, (view, row) radii "
          f"at the floor {floor:.3f}: {at_floor}, mean clipped fraction of the listed rows {clipped:.3f}, alpha {st['alpha']}")
    assert at_floor >= 1, "no radius at the floor"
    assert clipped > 0.5, "the clip is not active on many pixels"
    put("cfg", sc, out, inputs=False)

    W, H, ppm, V = 32, 32, 8.0, 2
    sc = make_hard_scene(rng, rb, V, W, H, ppm)
    cfg_kw = dict(tile_size=16, max_splats_per_tile=16, logdet0=-16.0)
    out, st = run_case(rr, rb, sc, n_views=V, width=W, height=H, ppm=ppm, centre=(0.0, 0.0), bev_kw={}, cfg_kw=cfg_kw)
    fam, valid = sc["family"], sc["valid_mask"]
    cond = np.array([[np.linalg.cond(out["Sigmas_inv"][k, i]) if valid[i] else 0.0 for i in range(fam.size)]
                     for k in range(V)])
    print(f"hard: {fam.size} rows ({int(valid.sum())} valid), min margin {st['min_margin']:.2e} px, closed-form diff "
          f"{st['closed_form_diff']:.2e}")
    for f, name in enumerate(HARD_FAMILIES):
        rows = np.flatnonzero((fam == f) & valid)
        assert rows.size, f"family {name} is missing"
        print(f"  {name:13s} {rows.size:3d} rows, cond(Sigma') {cond[:, rows].min():.2e} .. {cond[:, rows].max():.2e}, "
              f"alpha {out['alphas'][rows].min():.6g} .. {out['alphas'][rows].max():.6g}")
    assert cond.max() <= 1e6, cond.max()
    rows = lambda name: np.flatnonzero((fam == HARD_FAMILIES.index(name)) & valid)   # noqa: E731
    s3 = np.sqrt(np.linalg.eigvalsh(sc["covariances"][rows("thin")])[:, 0])
    assert np.all((s3 > 0.4e-6) & (s3 < 2.5e-6)), s3
    assert cond[:, rows("needle")].min() >= 1e5 and cond[:, rows("needle")].max() <= 1e6
    hm, hr = out["means"][:, rows("huge")], out["radii"][:, rows("huge")]
    assert np.all(out["alphas"][rows("huge")] == 0.02) and np.all(hr == 2.0 / np.sqrt(1e-12))
    assert np.all(hm[..., 0] - hr < 0) and np.all(hm[..., 0] + hr > W) and np.all(hm[..., 1] - hr < 0) and \
        np.all(hm[..., 1] + hr > H), "a huge row reaches every tile"
    assert np.all(out["alphas"][rows("tiny")] == 1.0)
    for k in range(V):
        assert np.all(clip_fraction(out, k, W, H, 25.0)[rows("tiny")] == 1.0), "the clip is active at every pixel"
    assert np.all(sc["kappas"][rows("kappa0")] == 0.0) and np.all(out["shaded"][:, rows("kappa1e4")] == 0.0)
    assert out["shaded"][:, rows("kappa0")].any()
    vd = out["view_dirs"]
    dn = sc["directions"][rows("antiparallel")]
    dn = dn / np.linalg.norm(dn, axis=1, keepdims=True)
    assert np.all((dn @ vd.T).min(1) < -1.0 + 1e-12)
    assert not sc["directions"][rows("zero_dir")].any()
    cr = sc["colors"][rows("colour_range")]
    assert (cr < 0).any() and (cr > 1).any()
    ua = sc["covariances"][rows("ulp_asym")]
    assert np.all(ua[:, 0, 1] != ua[:, 1, 0]) and np.all(np.abs(ua[:, 0, 1] - ua[:, 1, 0]) <= np.spacing(np.abs(ua[:, 1, 0])))
    for name in ("thin", "needle", "tiny", "huge"):
        assert np.isin(rows(name), out["tile_indices"]).any(), f"no {name} row is listed"
    put("hard", sc, out)
    edges["hard_family"] = fam
    edges["hard_family_names"] = np.array(HARD_FAMILIES)

    sc = make_lattice_scene(rng)
    cap = 7
    out, st = run_case(rr, rb, sc, n_views=1, width=64, height=32, ppm=1.0, centre=(0.0, 0.0),
                       bev_kw=dict(phi_center_deg=0.0), cfg_kw=dict(tile_size=32, max_splats_per_tile=cap),
                       mirror_ties=True, with_tiles=False, check_closed_form=False)
    assert np.array_equal(out["means"][0], sc["positions"][:, :2] + np.array([32.0, 16.0])), "the lattice is not exact"
    assert np.all(out["radii"] > 64.0)
    sizes = []
    for tx in range(2):
        d2 = np.sort(((out["means"][0] - np.array([16.0 + 32.0 * tx, 16.0])) ** 2).sum(1))
        assert d2[cap - 1] == d2[cap], "the cap does not fall inside a tie group"
        _, c = np.unique(d2, return_counts=True)
        assert np.all(np.isin(c, (2, 4, 8))), c
        sizes.append(int((d2 == d2[cap]).sum()))
    print(f"lattice: {sc['positions'].shape[0]} rows, min margin {st['min_margin']:.2e} px, the cap {cap} falls inside tie "
          f"groups of {sizes} rows, lists {out['tile_indices'][0, 0].tolist()}")
    put("lattice", sc, out, tiles=False)
    save("render_edges.npz", edges)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--edges-only", action="store_true", help="write render_edges.npz only (reads render_main.npz)")
    a = ap.parse_args()
    pkg = os.path.join(a.reference, "fl_ws", "src", "fl_slam_poc", "fl_slam_poc")
    rb = load_by_path(pkg, os.path.join("common", "bev_pushforward.py"), "ref_bev_pushforward")
    rr = load_by_path(pkg, os.path.join("backend", "rendering.py"), "ref_rendering")
    if a.edges_only:
        edge_cases(rr, rb)
        return
    rng = np.random.default_rng(SEED)
    save("render_ops.npz", ops_fixture(rr, rb, rng))

    scene = make_main_scene(rng)
    base = dict(cfg_kw=dict(tile_size=32, max_splats_per_tile=16, logdet0=-16.0), n_views=3, width=80, height=48,
                ppm=8.0, centre=(0.0, 0.0))
    t0 = time.perf_counter()
    out, st = run_case(rr, rb, scene, check_closed_form=False, **base)
    wall = time.perf_counter() - t0
    out, st = run_case(rr, rb, scene, **base)
    cnt = out["tile_counts"]
    print(f"main: {scene['positions'].shape[0]} rows ({int(scene['valid_mask'].sum())} valid), reference wall time "
          f"{wall:.1f} s; min margin {st['min_margin']:.2e} px, closed-form diff {st['closed_form_diff']:.2e}, "
          f"cond {st['cond']:.1e}, alpha {st['alpha']}, counts {cnt.reshape(3, -1).tolist()}")
    big = int(np.flatnonzero(scene["role"] == 5)[0])
    tight = int(np.flatnonzero(scene["role"] == 6)[0])
    bm, br = out["means"][:, big], out["radii"][:, big]
    assert np.all(bm[:, 0] - br < 32) and np.all(bm[:, 0] + br > 64) and np.all(bm[:, 1] - br < 32) and \
        np.all(bm[:, 1] + br > 32), "the x 400 row reaches every tile"
    assert (cnt == 16).any() and (cnt < 16).any(), "a tile at the cap and one under it"
    assert (out["tile_indices"] == tight).any(), "the tight row is listed"
    twins = np.flatnonzero((scene["positions"] == scene["positions"][np.flatnonzero(scene["role"] == 4)[0]]).all(1))
    assert twins.size == 2 and np.any((out["tile_indices"] == twins[0]).any(-1) & (out["tile_indices"] == twins[1]).any(-1)), \
        "the tied rows are listed together"
    assert scene["valid_mask"][out["tile_indices"][out["tile_indices"] >= 0]].all()
    save("render_main.npz", {**{k: scene[k] for k in INPUTS + ("role",)}, **{k: out[k] for k in STAGE}})
    save("render_main_tiles.npz", {k: out[k] for k in TILES})

    out, st = run_case(rr, rb, scene, **{**base, "cfg_kw": dict(tile_size=8, max_splats_per_tile=16, logdet0=-16.0),
                                        "width": 40, "height": 24, "ppm": 4.0})
    print(f"tile8: min margin {st['min_margin']:.2e}, closed-form diff {st['closed_form_diff']:.2e}")
    save("render_tile8.npz", {k: out[k] for k in STAGE + TILES})

    out, st = run_case(rr, rb, scene, **{**base, "cfg_kw": dict(tile_size=32, max_splats_per_tile=64, logdet0=-16.0),
                                        "n_views": 1})
    print(f"cap64: min margin {st['min_margin']:.2e}, counts {out['tile_counts'].ravel().tolist()}")
    assert (out["tile_counts"] == 64).any() and (out["tile_counts"] < 64).any()
    save("render_cap64.npz", {k: out[k] for k in STAGE + TILES})

    band = dict(scene)
    band["valid_mask"] = scene["valid_mask"] & ~np.isin(scene["role"], (2, 5, 6))
    out, st = run_case(rr, rb, band, **{**base, "n_views": 1})
    print(f"band: counts {out['tile_counts'].ravel().tolist()}")
    assert (out["tile_counts"] == 0).any(), "an empty tile"
    small = {"band_valid_mask": band["valid_mask"]}
    small.update({f"band_{k}": out[k] for k in STAGE + TILES})

    one = int(np.flatnonzero(scene["role"] == 1)[0])
    n1 = {k: scene[k][one:one + 1] for k in INPUTS}
    n1["valid_mask"] = np.array([True])
    out, st = run_case(rr, rb, n1, **base)
    small.update({f"n1_{k}": n1[k] for k in INPUTS})
    small.update({f"n1_{k}": out[k] for k in STAGE + TILES})
    n0 = {k: scene[k][:0] for k in INPUTS}
    out, st = run_case(rr, rb, n0, **base)
    small.update({f"n0_{k}": n0[k] for k in INPUTS})
    small.update({f"n0_{k}": out[k] for k in STAGE + TILES})
    save("render_small.npz", small)

    # fBm on: negative and large world coordinates (a map far from the origin)
    centre = (-1234.5, 98765.25)
    n = 48
    fb = dict(positions=np.stack([centre[0] + rng.uniform(-5.0, 5.0, n), centre[1] + rng.uniform(-3.0, 3.0, n),
                                  rng.uniform(0.0, 0.5, n)], 1),
              covariances=surfel_covs(rng, n, (0.1, 0.4), (0.01, 0.04)),
              directions=rng.normal(size=(n, 3)) + np.array([0.0, -0.3, 1.5]), kappas=rng.uniform(0.2, 3.0, n),
              colors=rng.uniform(0.2, 1.0, (n, 3)), valid_mask=rng.uniform(size=n) > 0.1)
    out, st = run_case(rr, rb, fb, n_views=2, width=40, height=24, ppm=4.0, centre=centre,
                       cfg_kw=dict(tile_size=16, max_splats_per_tile=8, logdet0=-10.0), fbm_scale=0.15, fbm_seed=7)
    print(f"fbm: min margin {st['min_margin']:.2e}, counts {out['tile_counts'].ravel().tolist()}")
    save("render_fbm.npz", {**{k: fb[k] for k in INPUTS}, **{k: out[k] for k in STAGE + TILES}})

    edge_cases(rr, rb)


if __name__ == "__main__":
    main()
