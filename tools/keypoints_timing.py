#!/usr/bin/env python3
"""Timing of the keypoint detector at the node's frame size: a 640 x 480 rgb8 frame on the device (noisy blocks
of 16 px, the `vga` fixture of tests/keypoints_ref.py restated here), the default KeypointConfig, and a
640 x 480 float32 depth image for the feature operator behind it.  Timed in one process with stream events,
each route after its own warm-up, the median of REPEAT calls:

  detect            gcslam.keypoints.KeypointDetector.detect: the kernels and the 16-byte counts read-back
  queue             the kernels alone (KeypointDetector.queue: nothing is waited for inside the timed call)
  readback          the 16-byte pinned read-back and its wait alone, on an idle stream
  extract_detect    VisualFeatureExtractor.extract(depth, rgb, None, K): detector and feature operator chained
  extract_upload    the same keypoints passed as pageable numpy arrays: the only route before the detector
  extract_device    the same keypoints already on the device (the feature operator alone)
  pyramid_queue     the pyramid detector's kernels alone (PyramidDetector.queue, the default PyramidConfig: 8 levels
                    at 6 / 5); to be read against `queue`
  pyramid_detect    PyramidDetector.detect: the kernels and the 144-byte read-back of counts and level_counts
  extract_pyramid   VisualFeatureExtractor.extract(depth, rgb, None, K, keypoint_config=PyramidConfig()): pyramid
                    detector and feature operator chained
  grid              the grid detector (GridDetector, cell_size 32, redistribute on) beside the pyramid detector on
                    the same frame, 8 levels, at max_keypoints 4,096 and 512: `queue` (kernels alone) and `detect`
                    of both, alternating, two rounds; the medians of both rounds and grid / pyramid of their means
  describe          gcslam.descriptors.KeypointDescriber.queue on the grid detector's keypoints of the frame at
                    max_keypoints 512 and 4,096 (orientation and 256-bit descriptor; nothing is waited for inside the
                    timed call), and `describe_keypoints`, the cached route
  match             DescriptorMatcher.queue of the frame's descriptors against those of the frame moved by (5, 3)
                    pixels, 512 x 512 and 4,096 x 4,096 (nearest and second nearest of every row, one way), and
                    `match_descriptors` with its defaults (both ways, the filters and the result's length read back)
  match_gated       DescriptorMatcher.queue_gated of the same sets with the keypoints' positions and levels and the
                    default GateConfig (radius 16, one level apart), one way; to be read against `match_queue`
  match_pairs       `match_pairs` without a gate and with the default gate (both searches, the filters, the cross check
                    and the compaction on the device, one wait for the count); to be read against `match_descriptors`

--desc prints the describe and match lines and GridDetector's `queue` and `detect` at both sizes only; --grid-only the
GridDetector lines only (with GCSLAM_LIB naming a build of before the describer, for a same-session comparison).
--profile-desc K runs the describer's and the matcher's `queue` at max_keypoints K for a kernel trace; --profile-gate K
the matcher's `queue`, `queue_gated` and both `match_pairs`.  --no-gate leaves the gated routes out (with GCSLAM_LIB
naming a build of before them).

--profile runs `detect` only, --profile-pyramid `pyramid_detect` only and --profile-grid K the pyramid's and the
grid's `detect` at max_keypoints K, WARMUP + REPEAT times, for a kernel trace taken from outside.  Prints one
JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gc-slam_amd"), ROOT]

W, H, WARMUP, REPEAT = 640, 480, 20, 200


def frame(np):
    g = np.random.default_rng(20)
    colours = g.integers(0, 256, (H // 16, W // 16, 3))
    img = np.repeat(np.repeat(colours, 16, 0), 16, 1) + g.integers(-6, 7, (H, W, 3))
    rgb = np.clip(img, 0, 255).astype(np.uint8)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    depth = (3.0 + 0.002 * (x - 320.0) + 1e-5 * (y - 240.0) ** 2 + 0.01 * g.standard_normal((H, W))).astype(np.float32)
    return rgb, depth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--profile-pyramid", action="store_true")
    ap.add_argument("--profile-grid", type=int, default=0, metavar="K")
    ap.add_argument("--desc", action="store_true")
    ap.add_argument("--grid-only", action="store_true")
    ap.add_argument("--profile-desc", type=int, default=0, metavar="K")
    ap.add_argument("--profile-gate", type=int, default=0, metavar="K")
    ap.add_argument("--no-gate", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    from gcslam import keypoints as KP
    from gcslam import visual as V
    from gcslam.camera import PinholeIntrinsics

    rgb, depth = frame(np)
    rgb_d, depth_d = torch.from_numpy(rgb).cuda(), torch.from_numpy(depth).cuda()
    K = PinholeIntrinsics(500.0, 500.0, 320.0, 240.0)
    det = KP.KeypointDetector()
    pyr, pcfg = KP.PyramidDetector(), KP.PyramidConfig()
    ex = V.VisualFeatureExtractor(V.VisualFeatureConfig(response_soft_scale=1e-3))
    kp = det.detect(rgb_d)
    kp_host = tuple(k.cpu().numpy() for k in kp)

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
        ms.sort()
        return statistics.median(ms), (ms[len(ms) // 10], ms[-1 - len(ms) // 10])   # median, 10th .. 90th percentile

    if args.profile:
        for _ in range(WARMUP + REPEAT):
            det.detect(rgb_d)
        print(json.dumps(dict(profile_calls=WARMUP + REPEAT)))
        return

    if args.profile_pyramid:
        for _ in range(WARMUP + REPEAT):
            pyr.detect(rgb_d)
        print(json.dumps(dict(profile_calls=WARMUP + REPEAT)))
        return

    if args.profile_grid:
        p, g = KP.PyramidDetector(KP.PyramidConfig(max_keypoints=args.profile_grid)), \
            KP.GridDetector(KP.GridConfig(max_keypoints=args.profile_grid))
        for _ in range(WARMUP + REPEAT):
            p.detect(rgb_d)
            g.detect(rgb_d)
        print(json.dumps(dict(profile_calls=WARMUP + REPEAT, max_keypoints=args.profile_grid)))
        return

    def desc_lines(caps, grid_only=False, profile=False, gate=True, profile_gate=False):
        """The describe and match lines (and GridDetector's own) at every cap."""
        res = {}
        moved = torch.roll(rgb_d, (3, 5), (0, 1)).contiguous()
        for cap in caps:
            g = KP.GridDetector(KP.GridConfig(max_keypoints=cap))
            ka, kb = g.detect(rgb_d), g.detect(moved)
            r = dict(grid_counts=list(ka.counts), moved_counts=list(kb.counts))
            routes = [("grid_queue", lambda: g.queue(rgb_d)), ("grid_detect", lambda: g.detect(rgb_d))]
            if not grid_only:
                from gcslam import descriptors as D
                d = D.KeypointDescriber(D.DescriptorConfig(max_keypoints=cap))
                m = D.DescriptorMatcher(D.MatchConfig(cap, cap))
                da, db = d.describe(rgb_d, ka), d.describe(moved, kb)
                pairs = D.match_descriptors(da, db)
                r.update(valid=int((da.angle_bin >= 0).sum()), pairs=int(pairs[0].shape[0]))
                routes = [("describe_queue", lambda: d.queue(rgb_d, ka[0], ka[1], ka.level)),
                          ("describe_keypoints", lambda: D.describe_keypoints(rgb_d, ka, D.DescriptorConfig(max_keypoints=cap))),
                          ("match_queue", lambda: m.queue(da.desc, db.desc, da.angle_bin, db.angle_bin)),
                          ("match_descriptors", lambda: D.match_descriptors(da, db))] + routes
                if gate:
                    gated = D.match_pairs(da, db, ka, kb)
                    r.update(pairs_no_gate=int(D.match_pairs(da, db)[0].shape[0]), pairs_gated=int(gated[0].shape[0]))
                    routes = [("match_gated", lambda: m.queue_gated(da.desc, db.desc, ka, kb, q_bin=da.angle_bin, t_bin=db.angle_bin)),
                              ("match_pairs", lambda: D.match_pairs(da, db)),
                              ("match_pairs_gated", lambda: D.match_pairs(da, db, ka, kb))] + routes
            if profile_gate:
                for _ in range(WARMUP + REPEAT):
                    for name in ("match_queue", "match_gated", "match_pairs", "match_pairs_gated"):
                        dict(routes)[name]()
                torch.cuda.synchronize()
            elif profile:
                for _ in range(WARMUP + REPEAT):
                    dict(routes)["describe_queue"]()
                    dict(routes)["match_queue"]()
                torch.cuda.synchronize()
            else:
                for name, _ in routes:
                    r[name + "_ms"], r[name + "_ms_p10_p90"] = [], []
                for _ in range(2):
                    for name, fn in routes:
                        med, spread = timed(fn)
                        r[name + "_ms"].append(med)
                        r[name + "_ms_p10_p90"].append(spread)
            res[f"k{cap}"] = r
            g.close()
        return res

    if args.desc or args.grid_only or args.profile_desc or args.profile_gate:
        caps = (args.profile_desc or args.profile_gate,) if args.profile_desc or args.profile_gate else (512, 4096)
        out = dict(width=W, height=H, warmup=WARMUP, repeat=REPEAT, lib=os.environ.get("GCSLAM_LIB", "in-tree"))
        out.update(desc_lines(caps, args.grid_only, bool(args.profile_desc), not args.no_gate, bool(args.profile_gate)))
        print(json.dumps(out))
        return

    pinned = torch.empty(4, dtype=torch.int32).pin_memory()
    counts_d = torch.zeros(4, dtype=torch.int32, device="cuda")

    def readback():
        pinned.copy_(counts_d, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        ev.synchronize()

    pk = pyr.detect(rgb_d)
    out = dict(width=W, height=H, warmup=WARMUP, repeat=REPEAT, counts=list(kp.counts), pyramid_counts=list(pk.counts),
               pyramid_level_counts=[list(c) for c in pk.level_counts])
    for name, fn in (("detect", lambda: det.detect(rgb_d)),
                     ("queue", lambda: det.queue(rgb_d)),
                     ("readback", readback),
                     ("extract_detect", lambda: ex.extract(depth_d, rgb_d, None, K)),
                     ("extract_upload", lambda: ex.extract(depth_d, rgb_d, kp_host, K)),
                     ("extract_device", lambda: ex.extract(depth_d, rgb_d, kp, K)),
                     ("pyramid_queue", lambda: pyr.queue(rgb_d)),
                     ("pyramid_detect", lambda: pyr.detect(rgb_d)),
                     ("extract_pyramid", lambda: ex.extract(depth_d, rgb_d, None, K, keypoint_config=pcfg))):
        out[name + "_ms"], out[name + "_ms_p10_p90"] = timed(fn)
    for cap in (4096, 512):
        p, g = KP.PyramidDetector(KP.PyramidConfig(max_keypoints=cap)), KP.GridDetector(KP.GridConfig(max_keypoints=cap))
        pk, gk = p.detect(rgb_d), g.detect(rgb_d)
        res = dict(pyramid_counts=list(pk.counts), grid_counts=list(gk.counts), grid_level_counts=[list(c) for c in gk.level_counts])
        routes = (("pyramid_queue", lambda: p.queue(rgb_d)), ("grid_queue", lambda: g.queue(rgb_d)),
                  ("pyramid_detect", lambda: p.detect(rgb_d)), ("grid_detect", lambda: g.detect(rgb_d)))
        for name, _ in routes:
            res[name + "_ms"], res[name + "_ms_p10_p90"] = [], []
        for _ in range(2):
            for name, fn in routes:
                m, spread = timed(fn)
                res[name + "_ms"].append(m)
                res[name + "_ms_p10_p90"].append(spread)
        for k in ("queue", "detect"):
            res[k + "_ratio"] = sum(res[f"grid_{k}_ms"]) / sum(res[f"pyramid_{k}_ms"])
        out[f"grid_k{cap}"] = res
        p.close()
        g.close()
    out["desc"] = desc_lines((512, 4096))
    print(json.dumps(out))
    det.close()
    pyr.close()
    ex.close()


if __name__ == "__main__":
    main()
