#!/usr/bin/env python3
"""Time render_map_view's library call at the BEV15 sweep's shape: V = 15 views of 512 x 512 px (256 tiles
per view at tile 32, cap 64) over a synthetic surfel map of N rows spread over 40 m x 40 m, at
N = 21 x 1,024 (a default stencil view) and N = 64 x 4,096 (every tile of a full map), 5 % of the rows
invalid.  Per size: the one-call gcs_render_view, and its three kernels through their own entry points
(gcs_render_prepare, gcs_render_bin_tiles, gcs_render_tiles; each synchronises, so each carries one
launch and one stream sync).  Stream events around --calls calls after --warmup.  Prints one JSON line."""

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gc-slam_amd")]

EXTENT_M = 40.0


def make_map(n, seed):
    rng = np.random.default_rng(seed)
    pos = np.stack([rng.uniform(-0.5, 0.5, n) * EXTENT_M, rng.uniform(-0.5, 0.5, n) * EXTENT_M,
                    rng.uniform(0.0, 2.0, n)], 1)
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    Rm = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], 1),
                   np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], 1),
                   np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1)], 1)
    sig = np.stack([rng.uniform(0.05, 0.2, n), rng.uniform(0.05, 0.2, n), rng.uniform(0.005, 0.02, n)], 1)
    cov = np.einsum("nij,nj,nkj->nik", Rm, sig * sig, Rm)
    return dict(positions=pos, covariances=0.5 * (cov + cov.transpose(0, 2, 1)),
                directions=rng.normal(size=(n, 3)) + [0.0, 0.0, 1.0], kappas=rng.uniform(0.5, 20.0, n),
                colors=rng.uniform(0.0, 1.0, (n, 3)), valid_mask=rng.uniform(size=n) > 0.05)


def timed(torch, fn, calls, warmup):
    for _ in range(warmup):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(calls + 1)]
    ev[0].record()
    for k in range(calls):
        fn()
        ev[k + 1].record()
    torch.cuda.synchronize()
    ms = np.array([ev[k].elapsed_time(ev[k + 1]) for k in range(calls)])
    return dict(median_ms=round(float(np.median(ms)), 4), min_ms=round(float(ms.min()), 4),
                max_ms=round(float(ms.max()), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=15)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--rows", type=int, nargs="+", default=[21 * 1024, 64 * 4096])
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    import torch
    from gcslam import rendering as R
    assert torch.cuda.is_available(), "render_bench needs a HIP device"
    cfg, bev = R.SplatRenderingConfig(logdet0=-16.0), R.BEVPushforwardConfig(n_views=a.views)
    W = H = a.size
    P_pix, off, vd = R.view_geometry(bev, W, H, W / EXTENT_M, (0.0, 0.0))
    r = R.renderer_for(cfg)
    res = dict(views=a.views, width=W, height=H, tile_size=cfg.tile_size, cap=cfg.max_splats_per_tile, calls=a.calls,
               warmup=a.warmup, sizes=[])
    for n in a.rows:
        m = {k: torch.as_tensor(v, device="cuda:0") for k, v in make_map(n, a.seed).items()}
        rows = (m["positions"], m["covariances"], m["directions"], m["kappas"], m["colors"], m["valid_mask"])
        view = lambda: r.render_view(*rows, P_pix, off, vd, W, H)   # noqa: E731
        out = view()
        s = r.prepare(*rows, P_pix, off, vd)
        idx, cnt = r.bin_tiles(s["means"], None, W, H, radii=s["radii"])
        assert torch.equal(idx, out.tile_indices) and torch.equal(cnt, out.tile_counts)
        img = r.render_tiles(s["means"], s["Sigmas_inv"], s["alphas"], s["colors"], idx, cnt, W, H, image_layout=True)
        assert torch.equal(img, out.images)
        c = cnt.cpu().numpy()
        res["sizes"].append(dict(
            rows=n, tiles_at_cap=int((c == cfg.max_splats_per_tile).sum()), tiles_empty=int((c == 0).sum()),
            tiles=int(c.size), listed_mean=round(float(c.mean()), 2),
            render_view=timed(torch, view, a.calls, a.warmup),
            prepare=timed(torch, lambda: r.prepare(*rows, P_pix, off, vd), a.calls, a.warmup),
            bin_tiles=timed(torch, lambda: r.bin_tiles(s["means"], None, W, H, radii=s["radii"]), a.calls, a.warmup),
            render_tiles=timed(torch, lambda: r.render_tiles(s["means"], s["Sigmas_inv"], s["alphas"], s["colors"], idx,
                                                             cnt, W, H, image_layout=True), a.calls, a.warmup)))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
