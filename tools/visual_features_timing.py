#!/usr/bin/env python3
"""Timing of the visual feature operator at the node's frame size: a 640 x 480 float32 depth image with its
rgb8 image on the device, 512 keypoints, the node's default parameters.  Two routes to the device feature
dict gcs_camera_splats reads, timed in one process with stream events (3 warm-ups, median of 10):

  extract        gcslam.visual.extract_visual_features: the keypoints uploaded, one gcs_visual_features call
  upload route   today's route for features computed elsewhere: the twelve host arrays (here the extractor's own,
                 downloaded beforehand) through CameraSplatBuilder.device_features -- the pinned staging
                 buffer and one H2D copy; the node's host loop that would fill them is not in this figure

The library call alone (keypoints already on the device) and a call with 2048 keypoints, which runs the
selection kernels in front, are timed as well.  Prints one JSON line."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gc-slam_amd"), ROOT]

W, H, N_KEYPOINTS, WARMUP, REPEAT = 640, 480, 512, 3, 10


def main():
    import numpy as np
    import torch
    from gcslam import visual as V
    from gcslam.camera import CameraSplatBuilder, PinholeIntrinsics

    g = np.random.default_rng(0)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    depth = (3.0 + 0.002 * (x - 320.0) + 1e-5 * (y - 240.0) ** 2 + 0.01 * g.standard_normal((H, W))).astype(np.float32)
    depth[g.integers(0, H, 3000), g.integers(0, W, 3000)] = np.nan
    depth_d = torch.from_numpy(depth).cuda()
    rgb_d = torch.from_numpy(g.integers(0, 256, (H, W, 3), dtype=np.uint8)).cuda()
    K = PinholeIntrinsics(500.0, 500.0, 320.0, 240.0)

    def keypoints(n):
        return np.stack([g.uniform(0, W - 1, n), g.uniform(0, H - 1, n), g.uniform(0.0, 200.0, n)], 1).astype(np.float32)

    kp, kp4 = keypoints(N_KEYPOINTS), keypoints(4 * N_KEYPOINTS)
    kp_d = [torch.from_numpy(np.ascontiguousarray(kp[:, j])).cuda() for j in range(3)]
    ex = V.VisualFeatureExtractor()
    builder = CameraSplatBuilder()
    host = {k: v.cpu().numpy() for k, v in ex.extract(depth_d, rgb_d, kp, K).items()}

    def timed(fn):
        ms = []
        for i in range(WARMUP + REPEAT):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if i >= WARMUP:
                ms.append(a.elapsed_time(b))
        return statistics.median(ms), (min(ms), max(ms))

    out = dict(width=W, height=H, keypoints=N_KEYPOINTS, warmup=WARMUP, repeat=REPEAT,
               fitted=int(host["has_mu"].sum()), valid_depth=int((host["depth_Lambda_c"] > 0).sum()))
    out["extract_ms"], out["extract_ms_range"] = timed(lambda: ex.extract(depth_d, rgb_d, kp, K))
    out["upload_route_ms"], out["upload_route_ms_range"] = timed(lambda: builder.device_features(host))
    out["call_only_ms"], out["call_only_ms_range"] = timed(lambda: ex.extract(depth_d, rgb_d, kp_d, K))
    out["extract_2048_keypoints_ms"], out["extract_2048_keypoints_ms_range"] = timed(
        lambda: ex.extract(depth_d, rgb_d, kp4, K))
    print(json.dumps(out))
    ex.close()
    builder.close()


if __name__ == "__main__":
    main()
