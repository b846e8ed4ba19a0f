#!/usr/bin/env python3
"""Camera-splat fixture recorded from the reference's own numpy code (data only).

Runs where a checkout of the reference is present (never on the GPU box): imports
fl_slam_poc.frontend.sensors.lidar_camera_depth_fusion / splat_prep from it, runs
lidar_depth_evidence(return_diag=True) and splat_prep_fused on a synthetic scene, applies the node's
base-frame conversion (backend_node.py:1885-1918) and the camera slice in information form
(camera_batch_utils.py:23-86, measurement_batch.py:165-259; np.linalg.inv stands in for the JAX
builder, which needs jax) and writes tests/golden/camera_splats.npz.  The tests read only the .npz.

Scene (camera frame, pinhole 640 x 480): three planes in disjoint image regions with 5 mm noise
(about 4,000 points), a 600-point dense patch, 64 points behind the camera, an empty band at the top
of the image; 96 features; lidar_projection_radius_pix = 8.  Points are float32 values (PointCloud2
x, y, z are float32), stored as float32.
  case A: identity extrinsics (the kernel's base -> camera transform is exact)
  case B: a real R_base_camera / t_base_camera; the base-frame cloud is rounded to float32

The script asserts the conditions on the inputs under which a second implementation must reproduce
the reference's integer decisions (in-radius sets, the 64 nearest of a plane fit, the plane normal),
and fails otherwise.

Usage: python tests/golden/make_camera_splats.py --reference <reference checkout>
"""

import argparse
import dataclasses
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FX, FY, CX, CY = 400.0, 400.0, 320.0, 240.0
RADIUS = 8.0
N_FEATURES = 96
TIMESTAMP = 1234.5
EPS_LIFT = 1e-9      # GC_EPS_LIFT, constants.py:71
SEED = 3


def plane_points(rng, n, u_rng, v_rng, normal, d, sigma=0.005):
    """n points of the plane normal . x = d seen at uniformly drawn pixels, noise along the normal."""
    normal = np.asarray(normal, np.float64) / np.linalg.norm(normal)
    u = rng.uniform(*u_rng, n)
    v = rng.uniform(*v_rng, n)
    ray = np.stack([(u - CX) / FX, (v - CY) / FY, np.ones(n)], axis=1)
    s = d / (ray @ normal)
    return ray * s[:, None] + rng.normal(0.0, sigma, n)[:, None] * normal


WALL = (-0.2, -0.1, 1.0)     # z ~ 4 m, tilted
FLOOR = (0.0, 1.0, 0.15)     # y ~ 1.2 m below the camera
SIDE = (1.0, -0.05, 0.6)     # slanted wall on the right


def plane_depth(u, v, normal, d):
    normal = np.asarray(normal, np.float64) / np.linalg.norm(normal)
    ray = np.array([(u - CX) / FX, (v - CY) / FY, 1.0])
    return d / float(ray @ normal)


def make_scene(rng):
    wall_n = np.asarray(WALL) / np.linalg.norm(WALL)
    wall_d = float(wall_n @ np.array([0.0, 0.0, 4.0]))
    side_n = np.asarray(SIDE) / np.linalg.norm(SIDE)
    side_d = float(side_n @ np.array([1.6, 0.0, 5.0]))
    floor_n = np.asarray(FLOOR) / np.linalg.norm(FLOOR)
    floor_d = float(floor_n @ np.array([0.0, 1.2, 3.0]))
    planes = dict(wall=(wall_n, wall_d, (0.0, 440.0), (60.0, 300.0)),
                  side=(side_n, side_d, (440.0, 640.0), (60.0, 300.0)),
                  floor=(floor_n, floor_d, (0.0, 640.0), (300.0, 480.0)))
    pts = [plane_points(rng, 1700, planes["wall"][2], planes["wall"][3], wall_n, wall_d),
           plane_points(rng, 900, planes["side"][2], planes["side"][3], side_n, side_d),
           plane_points(rng, 1400, planes["floor"][2], planes["floor"][3], floor_n, floor_d),
           plane_points(rng, 600, (150.0, 194.0), (150.0, 184.0), wall_n, wall_d)]   # dense patch, 44 x 34 px
    behind = rng.uniform(-3.0, 3.0, (64, 3))
    behind[:, 2] = -rng.uniform(0.5, 6.0, 64)
    pts.append(behind)
    p = np.concatenate(pts)
    p = p[rng.permutation(p.shape[0])]       # no structure in the point order
    return p.astype(np.float32).astype(np.float64), planes


def make_features(rng, planes):
    """96 features: 20 in the empty band, 8 inside the dense patch, the rest over the planes."""
    uv = np.concatenate([
        np.stack([rng.uniform(20, 620, 20), rng.uniform(5, 45, 20)], axis=1),
        np.stack([rng.uniform(160, 184, 8), rng.uniform(160, 174, 8)], axis=1),
        np.stack([rng.uniform(15, 625, 68), rng.uniform(75, 465, 68)], axis=1)])
    uv = uv[rng.permutation(N_FEATURES)]
    feats = []
    for i, (u, v) in enumerate(uv):
        if v < 60.0:
            z_true = 6.0
        elif v >= 300.0:
            z_true = plane_depth(u, v, *planes["floor"][:2])
        elif u >= 440.0:
            z_true = plane_depth(u, v, *planes["side"][:2])
        else:
            z_true = plane_depth(u, v, *planes["wall"][:2])
        sigma_c = 0.03 + 0.01 * z_true
        z_c = z_true + rng.normal(0.0, sigma_c)
        has_depth = i % 5 != 0                    # one feature in five: no camera depth (Lambda_c = 0)
        Lc = 1.0 / sigma_c ** 2 if has_depth else 0.0
        th = Lc * z_c
        mu = rng.normal(size=3)
        mu /= np.linalg.norm(mu)
        feats.append(dict(u=float(u), v=float(v), z_c=float(z_c), var_z=float(sigma_c ** 2 if has_depth else 1.0),
                          Lc=float(Lc), thc=float(th), weight=float(rng.uniform(0.2, 1.0)),
                          kappa=float(rng.uniform(1.0, 50.0)), mu=mu, has_mu=i % 3 != 1,
                          color=rng.uniform(-0.1, 1.1, 3), has_color=i % 4 != 2))
    return feats


def run_case(ref, p_base, R, t, feats, cfg, soft=False):
    """soft: the plane-fit conditions (eigen-gap, |n_z|) are recorded per feature as plane_determined,
    with Route B's intermediate z_raw / sigma^2 before its clamp / n . ray, and not asserted (the edge
    fixtures of make_camera_splats_edges.py keep undetermined features and compare them on everything
    that does not pass through the eigenvector)."""
    F = ref["fusion"]
    intr = ref["types"].PinholeIntrinsics(FX, FY, CX, CY)
    if p_base.shape[0] > 0:      # backend_node.py:1874-1878
        p_cam = (R.T @ (p_base.T - t[:, None])).T
    else:
        p_cam = np.zeros((0, 3))
    feat_in = []
    for f in feats:
        xyz = F.backproject_camera(f["u"], f["v"], f["z_c"], FX, FY, CX, CY)
        cov = F.backprojection_cov_camera(f["u"], f["v"], f["z_c"], 1.0, 1.0, f["var_z"], FX, FY, CX, CY)
        info = np.linalg.inv(cov + 1e-9 * np.eye(3))
        feat_in.append(ref["types"].Feature3D(
            u=f["u"], v=f["v"], xyz=xyz, cov_xyz=cov, info_xyz=info, logdet_cov=0.0, canonical_theta=info @ xyz,
            canonical_log_partition=0.0, desc=np.zeros(32, np.uint8), weight=f["weight"],
            meta={"depth_Lambda_c": f["Lc"], "depth_theta_c": f["thc"]},
            mu_app=f["mu"].copy() if f["has_mu"] else None, kappa_app=f["kappa"],
            color=f["color"].copy() if f["has_color"] else None))
    uvq = np.array([[f["u"], f["v"]] for f in feats])
    # the reference's own medians, recorded as it computes them (Route A calls np.median twice per
    # feature that has at least lidar_plane_fit_min_points candidates: z_med, then the MAD)
    rec = []
    real_median = np.median

    def spy(a, *args, **kw):
        out = real_median(a, *args, **kw)
        rec.append((int(np.size(a)), float(out)))
        return out

    np.median = spy
    try:
        Lam_ell, th_ell, diag = F.lidar_depth_evidence(p_cam, uvq, FX, FY, CX, CY, cfg, return_diag=True)
    finally:
        np.median = real_median
    # candidate sets by the reference's own projection and its in-radius expression (:122-140)
    uv, z = F._project_camera(p_cam, FX, FY, CX, CY)
    keep = z > 0.0
    uv, z, pk = uv[keep], z[keep], p_cam[keep]
    assert z.size == 0 or np.abs(z).min() >= 1e-9, "a kept point has |z| < 1e-9"
    M = len(feats)
    n_pt = np.zeros(M, np.int32)
    z_med, mad = np.full(M, np.nan), np.full(M, np.nan)
    r2 = cfg.lidar_projection_radius_pix * cfg.lidar_projection_radius_pix
    gap_min, ray_gap_min, nz_min = np.inf, np.inf, np.inf
    determined = np.ones(M, bool)
    z_raw, sig_raw, ndotr = np.full(M, np.nan), np.full(M, np.nan), np.full(M, np.nan)
    k = 0
    for i in range(M):
        d2 = (uv[:, 0] - uvq[i, 0]) ** 2 + (uv[:, 1] - uvq[i, 1]) ** 2
        assert d2.size == 0 or np.abs(d2 - r2).min() >= 1e-9 * r2, f"feature {i}: a point within 1e-9 r^2 of the radius"
        inr = d2 <= r2
        n_pt[i] = int(inr.sum())
        if n_pt[i] < cfg.lidar_plane_fit_min_points:
            continue
        assert rec[k][0] == n_pt[i] and rec[k + 1][0] == n_pt[i], "median call sequence"
        z_med[i], mad[i] = rec[k][1], rec[k + 1][1]
        k += 2
        near = pk[inr]
        ray = F.ray_from_pixel(uvq[i, 0], uvq[i, 1], FX, FY, CX, CY)
        dr = np.sort(F._distance_point_to_ray(near, ray))
        ku = min(cfg.lidar_ray_plane_fit_max_points, near.shape[0])
        if near.shape[0] > ku:
            ray_gap_min = min(ray_gap_min, (dr[ku] - dr[ku - 1]) / dr[ku])
        idx = np.argpartition(F._distance_point_to_ray(near, ray), ku - 1)[:ku]
        cen, normal, ev, sperp = F._fit_plane_weighted(near[idx], None)
        gap_min = min(gap_min, (ev[1] - ev[0]) / ev[2])
        nz_min = min(nz_min, abs(normal[2]))
        determined[i] = (ev[1] - ev[0]) / ev[2] >= 1e-3 and abs(normal[2]) >= 1e-6
        nr = float(np.dot(normal, ray))       # :316-326
        ndotr[i] = nr
        z_raw[i] = float(np.dot(normal, cen)) / (nr + cfg.plane_intersection_delta)
        sig_raw[i] = cfg.lidar_depth_base_sigma_m ** 2 + sperp / max(nr * nr + cfg.plane_intersection_delta,
                                                                      cfg.plane_intersection_delta)
    assert k == len(rec)
    assert ray_gap_min >= 1e-6, f"64th / 65th ray distances within {ray_gap_min:.2e}"
    if not soft:
        assert gap_min >= 1e-3, f"a plane fit has (lam2 - lam1) / lam3 = {gap_min:.2e}"
        assert nz_min >= 1e-6, "a plane normal has |n_z| < 1e-6 (its sign rule would be ill-conditioned)"

    fused = ref["prep"].splat_prep_fused(ref["types"].ExtractionResult(feat_in, [], int(TIMESTAMP * 1e9)), p_cam,
                                         intr, cfg)
    is_fused = np.array([g is not f for g, f in zip(fused, feat_in)])
    z_f = np.array([g.meta["depth_m"] if fu else 0.0 for g, fu in zip(fused, is_fused)])
    cam_xyz = np.array([g.xyz for g in fused])
    cam_cov = np.array([g.cov_xyz for g in fused])
    # backend_node.py:1887-1918
    base_xyz = np.array([R @ g.xyz + t for g in fused])
    base_cov = np.array([R @ np.asarray(g.cov_xyz).reshape(3, 3) @ R.T for g in fused])
    # camera_batch_utils.py:39-65 + measurement_batch.py:198-243, all rows (the tests cut at n_feat)
    dirs = np.zeros((M, 3))
    colors = np.zeros((M, 3))
    for i, g in enumerate(fused):
        d = R @ g.mu_app if g.mu_app is not None else base_xyz[i]
        dirs[i] = d / (np.linalg.norm(d) + 1e-12)
        c = g.color if g.color is not None else np.array([0.5, 0.5, 0.5])
        colors[i] = np.clip(c, 0.0, 1.0)
    Lam = np.array([np.linalg.inv(S + EPS_LIFT * np.eye(3)) for S in base_cov])
    th = np.einsum("nij,nj->ni", Lam, base_xyz)
    eta0 = np.array([g.kappa_app for g in fused])[:, None] * dirs
    cond = max(np.linalg.cond(S + EPS_LIFT * np.eye(3)) for S in base_cov)
    info = dict(n_points=int(p_base.shape[0]), n_kept=int(keep.sum()), gap_min=float(gap_min),
                ray_gap_min=float(ray_gap_min), cond_max=float(cond), kept_input=int((~is_fused).sum()))
    out = dict(points_base=p_base.astype(np.float32), R_base_camera=R, t_base_camera=t, n_pt=n_pt, z_med=z_med,
               mad=mad, Lambda_A=diag["Lambda_A"], theta_A=diag["theta_A"], Lambda_B=diag["Lambda_B"],
               theta_B=diag["theta_B"], Lambda_ell=Lam_ell, theta_ell=th_ell, fused=is_fused, z_f=z_f,
               cam_xyz=cam_xyz, cam_cov=cam_cov, base_xyz=base_xyz, base_cov=base_cov, Lambdas=Lam, thetas=th,
               eta0=eta0, weights=np.array([g.weight for g in fused]), colors=colors)
    if soft:
        out.update(plane_determined=determined, z_raw=z_raw, sig_raw=sig_raw, ndotr=ndotr)
    assert np.array_equal(out["points_base"].astype(np.float64), p_base, equal_nan=True)
    return out, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference repository")
    ap.add_argument("--out", default=os.path.join(HERE, "camera_splats.npz"))
    ap.add_argument("--seed", type=int, default=SEED)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(a.reference, "fl_ws", "src", "fl_slam_poc"))
    from fl_slam_poc.frontend.sensors import lidar_camera_depth_fusion as F, splat_prep as P, visual_types as T
    ref = dict(fusion=F, prep=P, types=T)
    defaults = dataclasses.asdict(F.LidarCameraDepthFusionConfig())
    cfg = F.LidarCameraDepthFusionConfig(lidar_projection_radius_pix=RADIUS)

    rng = np.random.default_rng(a.seed)
    p_cam, planes = make_scene(rng)
    feats = make_features(rng, planes)
    I3, z3 = np.eye(3), np.zeros(3)
    # case B: camera optical axes (z forward, x right, y down) in a base frame (x forward, y left, z up),
    # tilted by a small rotation, with a lever arm
    R0 = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])
    w = np.array([0.03, -0.08, 0.05])
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
    RB = (np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K) @ R0
    tB = np.array([0.12, -0.03, 0.35])
    pB = ((RB @ p_cam.T).T + tB).astype(np.float32).astype(np.float64)

    save = dict(intrinsics=np.array([FX, FY, CX, CY]), radius=np.array(RADIUS), timestamp=np.array(TIMESTAMP),
                eps_lift=np.array(EPS_LIFT), pixel_sigma=np.array(1.0),
                cfg_names=np.array(list(defaults.keys())), cfg_values=np.array([float(v) for v in defaults.values()]),
                cfg_is_int=np.array([isinstance(v, int) for v in defaults.values()]),
                u=np.array([f["u"] for f in feats]), v=np.array([f["v"] for f in feats]),
                depth_Lambda_c=np.array([f["Lc"] for f in feats]), depth_theta_c=np.array([f["thc"] for f in feats]),
                weight=np.array([f["weight"] for f in feats]), kappa_app=np.array([f["kappa"] for f in feats]),
                mu_app=np.array([f["mu"] for f in feats]), has_mu=np.array([f["has_mu"] for f in feats]),
                color=np.array([f["color"] for f in feats]), has_color=np.array([f["has_color"] for f in feats]))
    for name, (pb, R, t) in dict(A=(p_cam, I3, z3), B=(pB, RB, tB)).items():
        out, info = run_case(ref, pb, R, t, feats, cfg)
        n = out["n_pt"]
        cls = [int((n == 0).sum()), int(((n >= 1) & (n <= 2)).sum()), int(((n >= 3) & (n <= 64)).sum()),
               int((n > 64).sum())]
        assert all(c > 0 for c in cls), f"case {name}: a candidate-count class is empty: {cls}"
        assert info["kept_input"] > 0, "no keep-the-input feature"
        print(f"case {name}: candidates 0 / 1-2 / 3-64 / >64 = {cls} (max {n.max()}), kept input "
              f"{info['kept_input']}, min eigen-gap {info['gap_min']:.2e}, min ray gap {info['ray_gap_min']:.2e}, "
              f"max cond {info['cond_max']:.2e}, kept points {info['n_kept']} / {info['n_points']}")
        if name == "A":   # incoming camera-frame xyz / cov of every feature (kept when fusion does not apply)
            save["xyz_in"] = np.array([F.backproject_camera(f["u"], f["v"], f["z_c"], FX, FY, CX, CY) for f in feats])
            save["cov_in"] = np.array([F.backprojection_cov_camera(f["u"], f["v"], f["z_c"], 1.0, 1.0, f["var_z"],
                                                                   FX, FY, CX, CY) for f in feats])
        save.update({f"{name}_{k}": v for k, v in out.items()})
    np.savez_compressed(a.out, **save)
    print(f"{a.out}: {os.path.getsize(a.out)} bytes")
    assert os.path.getsize(a.out) < 200 * 1024


if __name__ == "__main__":
    main()
