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

The script asserts, and fails otherwise, the conditions that make the fixtures decidable for a second
implementation:
  * each of the four overlap comparisons of every (row, tile, view) has a margin above 1e-6 px;
  * in each tile's sorted dist^2 list consecutive gaps are exactly 0 between bit-identical rows or
    above 1e-6 px^2;
  * the same reference render fed the closed-form 2 x 2 inverse instead of np.linalg.inv differs from
    the recorded image by less than 1e-8 (a tenth of the end-to-end bar);
  * the main scene has a tile over the cap and a tile under it, the band case an empty tile.

Usage: python tests/golden/make_render.py --reference <reference checkout>
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
             check_closed_form=True):
    """The declared composition through the reference's functions.  Returns the record of every stage."""
    cfg = rr.SplatRenderingConfig(**cfg_kw)
    bev = rb.BEVPushforwardConfig(n_views=n_views)
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
                        assert all(np.array_equal(means[t], means[tied[0]]) for t in tied)
                idx = rr.splat_indices_for_tile((oy, ox), tile, means, Sinv, cap, cfg.eps)
                out["tile_indices"][k, ty, tx, :idx.size] = rows[idx]
                out["tile_counts"][k, ty, tx] = idx.size
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
    out["params"] = np.array([n_views, width, height, ppm, centre[0], centre[1], fbm_scale, fbm_seed], np.float64)
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
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, f"{name}: {size} bytes"
    print(f"  wrote {name}: {size / 1024:.0f} KB")


STAGE = ("P_pix", "offsets", "view_dirs", "means", "Sigmas_inv", "radii", "alphas", "shaded", "fbm", "params",
         "cfg_names", "cfg_values")
TILES = ("tile_indices", "tile_counts", "tiles")
INPUTS = ("positions", "covariances", "directions", "kappas", "colors", "valid_mask")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    a = ap.parse_args()
    pkg = os.path.join(a.reference, "fl_ws", "src", "fl_slam_poc", "fl_slam_poc")
    rb = load_by_path(pkg, os.path.join("common", "bev_pushforward.py"), "ref_bev_pushforward")
    rr = load_by_path(pkg, os.path.join("backend", "rendering.py"), "ref_rendering")
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


if __name__ == "__main__":
    main()
