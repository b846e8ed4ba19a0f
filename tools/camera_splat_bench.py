#!/usr/bin/env python3
"""Time gcs_camera_splats at the workload's shape: M = 512 features against the N = 65,536 points of a
gcslam.synthetic scan, a forward camera with a 72 deg horizontal field of view (about a fifth of the
360 deg scan in view), the reference's default fusion config.

  python tools/camera_splat_bench.py                      # GPU: stream events around --calls calls
  python tools/camera_splat_bench.py --reference PATH     # CPU: the reference's splat_prep_fused, once,
                                                          # on the same inputs (no GPU needed)
Prints one JSON line."""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gc-slam_amd")]

FX, FY, CX, CY = 440.0, 440.0, 320.0, 240.0
R_BASE_CAMERA = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])   # optical z = base x
T_BASE_CAMERA = np.array([0.1, 0.0, 0.4])


def make_inputs(n_points, n_features, seed):
    from gcslam import synthetic
    pts = synthetic.make_scan(n_points, 0, seed=seed)["points"]
    rng = np.random.default_rng(seed + 1)
    m = n_features
    u, v = rng.uniform(10.0, 630.0, m), rng.uniform(120.0, 360.0, m)
    z_c = rng.uniform(2.0, 9.0, m)
    sig2 = (0.03 + 0.01 * z_c) ** 2
    xyz = np.stack([(u - CX) * z_c / FX, (v - CY) * z_c / FY, z_c], axis=1)
    cov = np.zeros((m, 3, 3))
    cov[:, 0, 0] = cov[:, 1, 1] = (z_c / FX) ** 2 + 1e-4
    cov[:, 2, 2] = sig2
    mu = rng.normal(size=(m, 3))
    mu /= np.linalg.norm(mu, axis=1, keepdims=True)
    feats = dict(u=u, v=v, depth_Lambda_c=1.0 / sig2, depth_theta_c=z_c / sig2, xyz=xyz, cov=cov,
                 weight=rng.uniform(0.2, 1.0, m), kappa_app=rng.uniform(1.0, 50.0, m), mu_app=mu,
                 color=rng.uniform(0.0, 1.0, (m, 3)))
    p_cam = (R_BASE_CAMERA.T @ (pts.T - T_BASE_CAMERA[:, None])).T
    uu = FX * p_cam[:, 0] / np.maximum(p_cam[:, 2], 1e-9) + CX
    vv = FY * p_cam[:, 1] / np.maximum(p_cam[:, 2], 1e-9) + CY
    in_view = (p_cam[:, 2] > 0) & (uu >= 0) & (uu < 640) & (vv >= 0) & (vv < 480)
    return pts, feats, p_cam, float(in_view.mean())


def run_reference(path, feats, p_cam):
    sys.path.insert(0, os.path.join(path, "fl_ws", "src", "fl_slam_poc"))
    from fl_slam_poc.frontend.sensors import lidar_camera_depth_fusion as F, splat_prep as P, visual_types as T
    fl = [T.Feature3D(u=float(feats["u"][i]), v=float(feats["v"][i]), xyz=feats["xyz"][i], cov_xyz=feats["cov"][i],
                      info_xyz=np.eye(3), logdet_cov=0.0, canonical_theta=np.zeros(3), canonical_log_partition=0.0,
                      desc=np.zeros(32, np.uint8), weight=float(feats["weight"][i]),
                      meta={"depth_Lambda_c": float(feats["depth_Lambda_c"][i]),
                            "depth_theta_c": float(feats["depth_theta_c"][i])},
                      mu_app=feats["mu_app"][i], kappa_app=float(feats["kappa_app"][i]), color=feats["color"][i])
          for i in range(feats["u"].shape[0])]
    t0 = time.perf_counter()
    out = P.splat_prep_fused(T.ExtractionResult(fl, [], 0), p_cam, T.PinholeIntrinsics(FX, FY, CX, CY),
                             F.LidarCameraDepthFusionConfig())
    return (time.perf_counter() - t0) * 1e3, len(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=65536)
    ap.add_argument("--features", type=int, default=512)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reference", default=None, help="reference checkout: time its splat_prep_fused on the CPU")
    a = ap.parse_args()
    pts, feats, p_cam, frac = make_inputs(a.points, a.features, a.seed)
    res = dict(points=a.points, features=a.features, in_view_fraction=round(frac, 4))
    if a.reference:
        ms, n = run_reference(a.reference, feats, p_cam)
        res.update(mode="reference_cpu", splat_prep_fused_ms=round(ms, 3), n_fused=n)
        print(json.dumps(res))
        return
    import torch
    from gcslam.camera import CameraSplatBuilder, PinholeIntrinsics
    assert torch.cuda.is_available(), "camera_splat_bench needs a HIP device (or --reference for the CPU timing)"
    bld = CameraSplatBuilder(max_points=a.points)
    fa = bld.device_features(feats)
    p = torch.as_tensor(pts, device="cuda:0")
    intr = PinholeIntrinsics(FX, FY, CX, CY)
    call = lambda diag=False: bld.build(fa, p, intr, R_BASE_CAMERA, T_BASE_CAMERA, 100.0, want_diag=diag)  # noqa: E731
    b = call(True)
    n_pt = b.camera_diag["n_pt"].cpu().numpy()
    for _ in range(a.warmup):
        call()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(a.calls + 1)]
    ev[0].record()
    for k in range(a.calls):
        call()
        ev[k + 1].record()
    torch.cuda.synchronize()
    ms = np.array([ev[k].elapsed_time(ev[k + 1]) for k in range(a.calls)])
    res.update(mode="gpu", call_ms_median=round(float(np.median(ms)), 4), call_ms_min=round(float(ms.min()), 4),
               call_ms_max=round(float(ms.max()), 4), calls=a.calls, warmup=a.warmup,
               n_camera_valid=b.n_camera_valid, candidates_mean=round(float(n_pt.mean()), 2),
               candidates_max=int(n_pt.max()), fused=int(b.camera_diag["fused"].sum().item()))
    print(json.dumps(res))
    bld.close()


if __name__ == "__main__":
    main()
