#!/usr/bin/env python3
"""Edge-case camera-splat fixtures recorded from the reference's own numpy code (data only).

A sibling of make_camera_splats.py (same usage, same recording through run_case with its np.median
spy; runs only where a checkout of the reference is present, never on the GPU box).  It writes
  tests/golden/camera_edges_scene.npz     the cloud, the features, the configs, the padded clouds' digests
  tests/golden/camera_edges_<case>.npz    what the reference gave, one file per case
and leaves camera_splats.npz alone.

Scene (camera frame, pinhole 640 x 480, float32 values):
  far wall     30 - 41.5 m, tilted                   u 0-200,    v 60-240    (z_raw - z_min > 20)
  mid wall     about 12 m, tilted                    u 200-440,  v 60-240
  side wall    about 5 m, slanted                    u 440-640,  v 60-240
  floor        y = 1.2 m, 2.5 - 48 m, |n . ray| from 0.025 (v = 250) to 0.5     v 250-480
  patch P1     2,600 points in 20 x 20 px, about 4 m   more than 1,024 candidates at radius 8
  patch P2     1,400 points in 24 x 24 px, about 8 m   257 - 1,024 candidates
  patch P3     1,200 points in 30 x 30 px on the plane z = 3 exactly (equal depths, mad == 0)
  64 points behind the camera, 8 all-NaN rows (a non-dense PointCloud2), the rest of the top band empty
Features (300): the principal point, pixels left and right of the image, the empty band, the patches,
the grazing rows of the floor, the upper edge of the walls (one or two candidates), the rest anywhere.

Cases: r8_A, r8_B (radius 8, identity / real extrinsics), r3_A (the reference's default config),
fit_A (16 fitted points, 5 minimum points, gamma_lidar 0.5, camera / LiDAR weights 0.7 / 1.3),
depth_A (depth_min_m 30, depth_sigma_max_sq 1e-3), r8_E (no LiDAR point at all; the run on a cloud
that lies wholly behind the camera is asserted identical).

The radius and ray-gap conditions of make_camera_splats.py are asserted; the plane-fit conditions are
recorded per feature (plane_determined).  The reference is also run on the padded clouds of
tests/camera_pad.py and every recorded output asserted bit-identical to the unpadded run.

Usage: python tests/golden/make_camera_splats_edges.py --reference <reference checkout>
"""

import argparse
import dataclasses
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_camera_splats as base          # noqa: E402
from camera_pad import PADDED_SIZES, digest, filler, pad_cloud   # noqa: E402

FX, FY, CX, CY = base.FX, base.FY, base.CX, base.CY
SEED = 11
N_FEATURES = 300
CONFIGS = dict(
    r8=dict(lidar_projection_radius_pix=8.0),
    r3=dict(),
    fit=dict(lidar_projection_radius_pix=8.0, lidar_ray_plane_fit_max_points=16, lidar_plane_fit_min_points=5,
             gamma_lidar=0.5, depth_fusion_weight_camera=0.7, depth_fusion_weight_lidar=1.3),
    depth=dict(lidar_projection_radius_pix=8.0, depth_min_m=30.0, depth_sigma_max_sq=1e-3))
CASES = (("r8", "A"), ("r8", "B"), ("r3", "A"), ("fit", "A"), ("depth", "A"))
CLASSES = ((0, 0), (1, 2), (3, 64), (65, 256), (257, 1024), (1025, 1 << 30))
MAX_UNDETERMINED = 0.20
RECORDED = ("n_pt", "z_med", "mad", "Lambda_A", "theta_A", "Lambda_B", "theta_B", "fused", "z_f", "Lambdas", "thetas",
            "eta0", "weights", "colors", "plane_determined", "z_raw", "sig_raw", "ndotr")


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


# plane name -> (unit normal, d) of normal . x = d
FAR = (unit((-1.0, 0.0, 1.0)), 54.0 / np.sqrt(2.0))            # z = 54 / (1 - x/z): 30 m at u = 0, 41.5 m at u = 200
MID = (unit(base.WALL), float(unit(base.WALL) @ np.array([0.0, 0.0, 12.0])))
SIDE = (unit(base.SIDE), float(unit(base.SIDE) @ np.array([1.6, 0.0, 5.0])))
FLOOR = (np.array([0.0, 1.0, 0.0]), 1.2)
P1 = (unit(base.WALL), float(unit(base.WALL) @ np.array([0.0, 0.0, 4.0])))
P2 = (unit((0.15, 0.1, 1.0)), float(unit((0.15, 0.1, 1.0)) @ np.array([0.0, 0.0, 8.0])))
P3_Z = 3.0
P1_BOX, P2_BOX, P3_BOX = ((350.0, 370.0), (15.0, 35.0)), ((420.0, 444.0), (12.0, 36.0)), ((500.0, 530.0), (10.0, 40.0))


def make_scene(rng):
    pp = base.plane_points
    pts = [pp(rng, 1200, (0.0, 200.0), (60.0, 240.0), *FAR),
           pp(rng, 1500, (200.0, 440.0), (60.0, 240.0), *MID),
           pp(rng, 900, (440.0, 640.0), (60.0, 240.0), *SIDE),
           pp(rng, 2500, (0.0, 640.0), (250.0, 480.0), *FLOOR),
           pp(rng, 2600, *P1_BOX, *P1),
           pp(rng, 1400, *P2_BOX, *P2)]
    u, v = rng.uniform(*P3_BOX[0], 1200), rng.uniform(*P3_BOX[1], 1200)
    pts.append(np.stack([(u - CX) / FX * P3_Z, (v - CY) / FY * P3_Z, np.full(1200, P3_Z)], axis=1))
    behind = rng.uniform(-3.0, 3.0, (64, 3))
    behind[:, 2] = -rng.uniform(0.5, 6.0, 64)
    pts.append(behind)
    pts.append(np.full((8, 3), np.nan))
    p = np.concatenate(pts)
    p = p[rng.permutation(p.shape[0])]
    return p.astype(np.float32).astype(np.float64)


def true_depth(u, v):
    """Depth of the surface a pixel sees (the camera depth of its feature is drawn around it)."""
    def on(box, margin=9.0):
        return box[0][0] - margin <= u <= box[0][1] + margin and box[1][0] - margin <= v <= box[1][1] + margin
    if on(P3_BOX):
        return P3_Z
    if on(P1_BOX):
        return base.plane_depth(u, v, *P1)
    if on(P2_BOX):
        return base.plane_depth(u, v, *P2)
    if v < 56.0:
        return 6.0
    if v >= 246.0:
        return base.plane_depth(u, max(v, 250.0), *FLOOR)
    uu = min(max(u, 0.0), 640.0)
    return base.plane_depth(uu, v, *(FAR if uu < 200.0 else MID if uu < 440.0 else SIDE))


def centre(box):
    return 0.5 * (box[0][0] + box[0][1]), 0.5 * (box[1][0] + box[1][1])


def around(rng, box, half, n):
    c = centre(box)
    return np.stack([rng.uniform(c[0] - half, c[0] + half, n), rng.uniform(c[1] - half, c[1] + half, n)], axis=1)


def make_features(rng):
    U = rng.uniform
    groups = [np.array([[CX, CY]]),                                                    # the principal point
              np.stack([U(-30.0, -4.0, 6), U(70.0, 470.0, 6)], axis=1),                # left of the image
              np.stack([U(644.0, 670.0, 6), U(70.0, 470.0, 6)], axis=1),               # right of it
              np.stack([U(20.0, 320.0, 20), U(5.0, 42.0, 20)], axis=1),                # the empty band
              around(rng, P1_BOX, 1.5, 6), around(rng, P1_BOX, 9.0, 12),
              around(rng, P2_BOX, 3.0, 12), around(rng, P2_BOX, 11.0, 6),
              around(rng, P3_BOX, 4.0, 8), around(rng, P3_BOX, 14.0, 8),
              np.stack([U(10.0, 630.0, 24), U(251.0, 275.0, 24)], axis=1),             # grazing floor
              np.stack([U(10.0, 630.0, 14), U(51.0, 54.5, 14)], axis=1)]               # just above the walls
    n = sum(g.shape[0] for g in groups)
    groups.append(np.stack([U(5.0, 635.0, N_FEATURES - n), U(65.0, 475.0, N_FEATURES - n)], axis=1))
    uv = np.concatenate(groups)
    uv = np.concatenate([uv[:1], uv[1:][rng.permutation(N_FEATURES - 1)]])    # feature 0: the principal point
    feats = []
    for i, (u, v) in enumerate(uv):
        z_true = true_depth(u, v)
        sigma_c = 0.03 + 0.01 * z_true
        z_c = z_true + rng.normal(0.0, sigma_c)
        has_depth = i % 5 != 0
        Lc = 1.0 / sigma_c ** 2 if has_depth else 0.0
        mu = rng.normal(size=3)
        mu /= np.linalg.norm(mu)
        feats.append(dict(u=float(u), v=float(v), z_c=float(z_c), var_z=float(sigma_c ** 2 if has_depth else 1.0),
                          Lc=float(Lc), thc=float(Lc * z_c), weight=float(rng.uniform(0.2, 1.0)),
                          kappa=float(rng.uniform(1.0, 50.0)), mu=mu, has_mu=i % 3 != 1,
                          color=rng.uniform(-0.1, 1.1, 3), has_color=i % 4 != 2))
    return feats


def class_counts(n, ok):
    return [int(((n >= lo) & (n <= hi) & ok).sum()) for lo, hi in CLASSES]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference repository")
    ap.add_argument("--out-dir", default=HERE)
    ap.add_argument("--seed", type=int, default=SEED)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(a.reference, "fl_ws", "src", "fl_slam_poc"))
    from fl_slam_poc.frontend.sensors import lidar_camera_depth_fusion as F, splat_prep as P, visual_types as T
    ref = dict(fusion=F, prep=P, types=T)
    defaults = dataclasses.asdict(F.LidarCameraDepthFusionConfig())
    cfgs = {k: F.LidarCameraDepthFusionConfig(**kw) for k, kw in CONFIGS.items()}
    assert cfgs["r3"] == F.LidarCameraDepthFusionConfig() and cfgs["r3"].lidar_projection_radius_pix == 3.0

    rng = np.random.default_rng(a.seed)
    p_cam = make_scene(rng)
    feats = make_features(rng)
    M = len(feats)
    assert 257 <= M <= 512
    I3, z3 = np.eye(3), np.zeros(3)
    R0 = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])       # case B of make_camera_splats.py
    w = np.array([0.03, -0.08, 0.05])
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
    RB = (np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K) @ R0
    tB = np.array([0.12, -0.03, 0.35])
    pB = ((RB @ p_cam.T).T + tB).astype(np.float32).astype(np.float64)
    ext = dict(A=(p_cam, I3, z3), B=(pB, RB, tB))

    scene = dict(intrinsics=np.array([FX, FY, CX, CY]), timestamp=np.array(base.TIMESTAMP),
                 eps_lift=np.array(base.EPS_LIFT), pixel_sigma=np.array(1.0), points=p_cam.astype(np.float32),
                 cfg_names=np.array(list(defaults.keys())),
                 cfg_defaults=np.array([float(v) for v in defaults.values()]),
                 cfg_is_int=np.array([isinstance(v, int) for v in defaults.values()]),
                 config_ids=np.array(list(CONFIGS)),
                 cfg_values=np.array([[float(getattr(cfgs[c], k)) for k in defaults] for c in CONFIGS]),
                 cases=np.array([f"{c}_{e}" for c, e in CASES] + ["r8_E"]),
                 u=np.array([f["u"] for f in feats]), v=np.array([f["v"] for f in feats]),
                 depth_Lambda_c=np.array([f["Lc"] for f in feats]), depth_theta_c=np.array([f["thc"] for f in feats]),
                 weight=np.array([f["weight"] for f in feats]), kappa_app=np.array([f["kappa"] for f in feats]),
                 mu_app=np.array([f["mu"] for f in feats]), has_mu=np.array([f["has_mu"] for f in feats]),
                 color=np.array([f["color"] for f in feats]), has_color=np.array([f["has_color"] for f in feats]),
                 xyz_in=np.array([F.backproject_camera(f["u"], f["v"], f["z_c"], FX, FY, CX, CY) for f in feats]),
                 cov_in=np.array([F.backprojection_cov_camera(f["u"], f["v"], f["z_c"], 1.0, 1.0, f["var_z"],
                                                              FX, FY, CX, CY) for f in feats]))
    assert np.array_equal(scene["points"].astype(np.float64), p_cam, equal_nan=True)

    outs = {}
    for c, e in CASES:
        pb, R, t = ext[e]
        out, info = base.run_case(ref, pb, R, t, feats, cfgs[c], soft=True)
        n, det = out["n_pt"], out["plane_determined"]
        runs_b = np.isfinite(out["z_raw"])
        und = int((runs_b & ~det).sum())
        print(f"case {c}_{e}: candidates {class_counts(n, np.ones(M, bool))} (determined {class_counts(n, det)}), "
              f"max {n.max()}, Route B on {int(runs_b.sum())}, undetermined {und}, kept input "
              f"{info['kept_input']}, min ray gap {info['ray_gap_min']:.2e}, max cond {info['cond_max']:.2e}, "
              f"kept points {info['n_kept']} / {info['n_points']}")
        assert und <= MAX_UNDETERMINED * runs_b.sum(), f"{c}_{e}: {und} of {runs_b.sum()} Route-B features undetermined"
        outs[f"{c}_{e}"] = out
    # coverage the tests rely on (asserted again over the committed files by tests/test_camera_edges_host.py)
    for name in ("r8_A", "r8_B"):
        cc = class_counts(outs[name]["n_pt"], outs[name]["plane_determined"])
        assert all(x >= 3 for x in cc), f"{name}: a candidate class has fewer than three determined features: {cc}"
    o = outs["r8_A"]
    assert int((o["mad"] == 0.0).sum()) >= 3, "fewer than three features with equal candidate depths"
    assert int(((o["mad"] == 0.0) & (o["n_pt"] > 256)).sum()) >= 1, "no equal-depth feature with more than 256 candidates"
    det = o["plane_determined"]
    x = o["z_raw"] - cfgs["r8"].depth_min_m
    assert (det & (x > 20.0)).any(), "no determined feature with z_raw - z_min > 20"
    assert (det & (np.abs(o["ndotr"]) < 0.05)).any() and (det & (np.abs(o["ndotr"]) > cfgs["r8"].plane_angle_sigmoid_t)).any()
    o = outs["depth_A"]
    det, x = o["plane_determined"], o["z_raw"] - cfgs["depth"].depth_min_m
    assert (det & (x < -20.0)).any() and (det & (x < 0.0) & (x >= -20.0)).any() and (det & (x > 0.0)).any()
    assert (det & (o["sig_raw"] > cfgs["depth"].depth_sigma_max_sq)).any(), "no determined feature with a clamped sigma"
    o = outs["fit_A"]
    assert ((o["n_pt"] > 16) & o["plane_determined"]).sum() >= 3 and ((o["n_pt"] >= 3) & (o["n_pt"] < 5)).sum() >= 1

    # no LiDAR at all, and a cloud wholly behind the camera: the same recorded outputs
    out_e, _ = base.run_case(ref, np.zeros((0, 3)), I3, z3, feats, cfgs["r8"], soft=True)
    behind = filler(512)[::2].astype(np.float64)
    assert (behind[:, 2] < 0).all()
    out_h, _ = base.run_case(ref, behind, I3, z3, feats, cfgs["r8"], soft=True)
    for k in RECORDED:
        assert same_bits(out_e[k], out_h[k]), f"behind-only cloud: {k} differs from the empty cloud's"
    outs["r8_E"] = out_e

    # padded clouds: the reference's outputs are those of the stored cloud, bit for bit
    digests = []
    for n_total in PADDED_SIZES:
        cloud = pad_cloud(scene["points"], n_total)
        out_p, info = base.run_case(ref, cloud.astype(np.float64), I3, z3, feats, cfgs["r8"], soft=True)
        for k in RECORDED:
            assert same_bits(out_p[k], outs["r8_A"][k]), f"padded to {n_total}: {k} differs"
        assert info["n_points"] == n_total
        digests.append(digest(cloud))
        print(f"padded to {n_total}: identical outputs, kept points {info['n_kept']}, sha256 {digests[-1][:16]}...")
    scene["padded_sizes"] = np.array(PADDED_SIZES)
    scene["padded_sha256"] = np.array(digests)

    def write(name, d):
        path = os.path.join(a.out_dir, name)
        np.savez_compressed(path, **d)
        print(f"{path}: {os.path.getsize(path)} bytes")
        assert os.path.getsize(path) < 200 * 1024

    write("camera_edges_scene.npz", scene)
    for name, out in outs.items():
        d = {k: out[k] for k in RECORDED + ("R_base_camera", "t_base_camera")}
        if name.endswith("_B"):
            d["points_base"] = out["points_base"]
        write(f"camera_edges_{name}.npz", d)


if __name__ == "__main__":
    main()
