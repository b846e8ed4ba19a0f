"""Wall time of a live-path scan that carries camera features, at bench.py's live_path sizes
(PipelineConfig defaults: N_POINTS_CAP 8,192, m_tile 50,000, 7 active / stencil tiles, n_feat 512 +
n_surfel 1,024), with the 96 features of tests/golden/camera_splats.npz (case B's camera) or 512 tiled
from them, over consecutive synthetic scans.  Three ways, each on its own (context, map) over the same
scans, warm-up then the median of the timed calls, as bench.py does:

  a  camera_batch_from_features on the scan's points, then process_scan_single_hypothesis with the batch
     (timed together: what a caller without CameraFrame does per scan)
  b  process_scan_single_hypothesis with a batch built beforehand (gcs_live_scan_camera's form B)
  c  process_scan_single_hypothesis with a CameraFrame (form A: the slice is built inside the call)
  l  no camera batch: the LiDAR-only chain, for scale

Mode a uses only what a tree without CameraFrame has, so the same file times that tree too
(--modes a).  One JSON line per (mode, feature count)."""

import argparse
import gc
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gc-slam_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def fixture_features(m):
    fx = dict(np.load(os.path.join(ROOT, "tests", "golden", "camera_splats.npz")))
    names = dict(u="u", v="v", depth_Lambda_c="depth_Lambda_c", depth_theta_c="depth_theta_c", xyz="xyz_in",
                 cov="cov_in", weight="weight", kappa_app="kappa_app", mu_app="mu_app", has_mu="has_mu",
                 color="color", has_color="has_color")
    reps = -(-m // fx["u"].shape[0])
    feats = {k: np.concatenate([fx[v]] * reps)[:m] for k, v in names.items()}
    return feats, fx


def run(mode, m, steps, warmup, device):
    import torch
    from gcslam import pipeline as GP, primitive_map as gpm, synthetic
    from gcslam.camera import DepthFusionConfig, PinholeIntrinsics, camera_batch_from_features
    N = 8192
    cfg = GP.PipelineConfig(K_HYP=1, N_POINTS_CAP=N, B_BINS=48, soft_assign_mode="dense",
                            lidar_origin_base=tuple(synthetic.LIDAR_ORIGIN), max_raw_points=N, device=device,
                            camera_batch_policy="use")
    ctx = cfg.make_context()
    am = gpm.create_empty_atlas_map(m_tile=cfg.primitive_map_max_size, max_tiles=512, device=device)
    Q = GP.process_noise_state_to_Q(GP.datasheet_process_noise_state())
    scans = [synthetic.make_scan(N, k) for k in range(warmup + steps)]
    feats, fx = fixture_features(m)
    K = PinholeIntrinsics(*fx["intrinsics"])
    R, t, ts = fx["B_R_base_camera"], fx["B_t_base_camera"], float(fx["timestamp"])
    fusion = DepthFusionConfig(lidar_projection_radius_pix=float(fx["radius"]))

    def build(sc):
        return camera_batch_from_features(feats, sc["points"], K, R, t, ts, config=fusion, n_feat=cfg.n_feat,
                                          n_surfel=cfg.n_surfel, eps_lift=cfg.eps_lift, device=device)

    state = dict(belief=GP.BeliefGaussianInfo.create_identity_prior(), seq=0)
    prebuilt = build(scans[0]) if mode == "b" else None

    def one(sc):
        if mode == "a":
            cam = build(sc)
        elif mode == "b":
            cam = prebuilt
        elif mode == "c":
            from gcslam.camera import CameraFrame
            cam = CameraFrame(feats, K, R, t, ts, config=fusion)
        else:
            cam = None
        r = GP.process_scan_single_hypothesis(
            belief_prev=state["belief"], raw_points=sc["points"], raw_timestamps=sc["timestamps"],
            raw_weights=sc["weights"], raw_ring=None, raw_tag=None, imu_stamps=sc["imu_stamps"],
            imu_gyro=sc["imu_gyro"], imu_accel=sc["imu_accel"], odom_pose=sc["odom_pose"],
            odom_cov_se3=sc["odom_cov_se3"], scan_start_time=sc["scan_start_time"], scan_end_time=sc["scan_end_time"],
            dt_sec=sc["dt_sec"], t_last_scan=sc["t_last_scan"], t_scan=sc["t_scan"], Q=Q, config=cfg,
            odom_twist=sc["odom_twist"], odom_twist_cov=sc["odom_twist_cov"], camera_batch=cam,
            scan_seq=state["seq"], primitive_map=am, map_bins=ctx)
        state["belief"] = r.belief_updated
        state["seq"] += 1
        return r

    for k in range(warmup):
        one(scans[k])
    torch.cuda.synchronize()
    gc.collect()
    gc.freeze()
    stamps_prev = GP._STAMPS_ON
    GP._STAMPS_ON = True   # the chain's phase_us land in GP.LIVE_PHASES
    GP.LIVE_PHASES.clear()
    per = np.zeros(steps)
    n_cam = 0
    for i in range(steps):
        t0 = time.perf_counter()
        r = one(scans[warmup + i])
        per[i] = time.perf_counter() - t0
        n_cam = int(r.measurement_batch.n_camera_valid)
    GP._STAMPS_ON = stamps_prev
    gc.unfreeze()
    out = dict(mode=mode, n_features=m, n_camera_valid=n_cam, steps=steps, warmup=warmup,
               ms_median=round(float(np.median(per)) * 1e3, 4), ms_p10=round(float(np.percentile(per, 10)) * 1e3, 4),
               ms_p90=round(float(np.percentile(per, 90)) * 1e3, 4), ms_min=round(float(per.min()) * 1e3, 4))
    if GP.LIVE_PHASES:   # the one-call chain ran: median host clock of each phase mark (us since entry)
        ph = np.median(np.array(GP.LIVE_PHASES), axis=0)
        out["phase_us"] = [round(float(x), 1) for x in ph]
        out["path"] = "chain"
    else:
        out["path"] = "per-operator"
    ctx.close()
    am.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--modes", default="a,b,c,l")
    ap.add_argument("--features", default="96,512")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    for m in (int(x) for x in a.features.split(",")):
        for mode in a.modes.split(","):
            if mode == "l" and m != int(a.features.split(",")[0]):
                continue
            print(json.dumps(run(mode, m, a.steps, a.warmup, a.device)), flush=True)


if __name__ == "__main__":
    main()
