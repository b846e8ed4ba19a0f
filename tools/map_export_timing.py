#!/usr/bin/env python3
"""Timing of map publishing at the reference sizes: 7 stencil tiles of m_tile = 50,000 slots
(GC_PRIMITIVE_MAP_MAX_SIZE) at 60 % occupancy, newest first.  Two routes to the same published bytes and
renderable batch, timed in one process with stream events (3 warm-ups, median of 10):

  publish_map   gcslam.map_export.publish_map: one gcs_pmap_export call, then the records copied to the host
  view route    what a caller could do before that call existed: extract_atlas_map_view with
                m_tile_view = m_tile (the padded, weight-ordered view), then on the device with torch the
                valid-row mask, the two stable sorts (id, then negated recency), the batched inverse of
                Sigma + eps I and the float32 packing, then the same copy to the host

The view route's stages are timed one by one as well, and the library call without the host copy.  Prints
one JSON line."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gc-slam_amd"), ROOT]

M_TILE, N_TILES, OCCUPANCY, WARMUP, REPEAT = 50000, 7, 0.6, 3, 10
EPS_LIFT = 1e-9


def build_map(rng):
    import numpy as np
    from gcslam.primitive_map import AtlasMap
    from oracle import primitive_map as opm
    am = AtlasMap(m_tile=M_TILE, max_tiles=N_TILES, max_merge=0)
    tids = [(1 << 40) + 17 * k for k in range(N_TILES)]
    for k, tid in enumerate(tids):
        t = opm.create_empty_tile(M_TILE)
        t["valid_mask"][:] = rng.random(M_TILE) < OCCUPANCY
        t["weights"][:] = rng.random(M_TILE) * 2.0
        A = rng.normal(size=(M_TILE, 3, 3)) * 0.3
        t["Lambdas"][:] = np.einsum("nij,nkj->nik", A, A) + np.eye(3)[None] * 2.0
        t["thetas"][:] = rng.normal(size=(M_TILE, 3)) * 3.0
        t["etas"][:] = rng.normal(size=(M_TILE, 3, 3))
        t["last_supported_scan_seq"][:] = rng.integers(0, 400, M_TILE)
        t["primitive_ids"][:] = k * M_TILE + rng.permutation(M_TILE)
        t["rgb"][:] = rng.random((M_TILE, 3))
        am.write_tile(tid, t)
    return am, tids


def main():
    import numpy as np
    import torch
    from gcslam import map_export as ME
    from gcslam.primitive_map import extract_atlas_map_view

    am, tids = build_map(np.random.default_rng(0))
    eye = EPS_LIFT * torch.eye(3, dtype=torch.float64, device="cuda")

    spread = []   # (min, max) of each timed() in call order

    def timed(fn):
        ms = []
        for i in range(WARMUP + REPEAT):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = fn()
            b.record()
            b.synchronize()
            if i >= WARMUP:
                ms.append(a.elapsed_time(b))
        spread.append((min(ms), max(ms)))
        return statistics.median(ms), out

    def view():
        return extract_atlas_map_view(am, tids, M_TILE, EPS_LIFT)

    def mask(v):
        k = v.valid_mask
        return {f: getattr(v, f)[k] for f in ("positions", "covariances", "weights", "etas", "colors", "primitive_ids",
                                              "last_supported_scan_seq", "directions", "kappas")}

    def sort(r):
        o = torch.sort(r["primitive_ids"], stable=True).indices
        o = o[torch.sort(-r["last_supported_scan_seq"][o], stable=True).indices]
        return {f: x[o] for f, x in r.items()}

    def inverse(r):
        return torch.linalg.inv(r["covariances"] + eye)

    def pack(r):
        return torch.cat([r["positions"].to(torch.float32),
                          torch.clamp(r["weights"].to(torch.float32), 0.0, 1e6)[:, None]], dim=1)

    def view_route():
        r = sort(mask(view()))
        lw = inverse(r)
        return pack(r).cpu().numpy().tobytes(), r, lw

    out = dict(m_tile=M_TILE, n_tiles=N_TILES, occupancy=OCCUPANCY, warmup=WARMUP, repeat=REPEAT)
    out["publish_map_ms"], (cloud, batch) = timed(lambda: ME.publish_map(am, tids, None, EPS_LIFT))
    out["view_route_ms"], (data, rows, lw) = timed(view_route)
    out["rows"] = cloud.width
    out["publish_map_ms_range"], out["view_route_ms_range"] = spread[0], spread[1]
    out["export_call_ms"], _ = timed(lambda: ME.export_rows(am, tids, None, ME.ORDER_RECENCY, EPS_LIFT,
                                                             fields=ME._BATCH_FIELDS))
    out["view_ms"], v = timed(view)
    out["mask_ms"], r = timed(lambda: mask(v))
    out["sort_ms"], s = timed(lambda: sort(r))
    out["inverse_ms"], _ = timed(lambda: inverse(s))
    out["pack_copy_ms"], _ = timed(lambda: pack(s).cpu().numpy().tobytes())
    # the two routes publish the same rows in the same order
    same_order = torch.equal(rows["primitive_ids"], batch.primitive_ids)
    a, b = np.frombuffer(data, "<f4"), np.frombuffer(cloud.data, "<f4")
    out["same_order"], out["same_bytes"] = bool(same_order), bool(len(a) == len(b) and a.tobytes() == b.tobytes())
    out["lambda_world_max_rel_diff"] = float(((lw - batch.Lambda_world).abs().amax() / lw.abs().amax()).cpu())
    print(json.dumps(out))
    am.close()


if __name__ == "__main__":
    main()
