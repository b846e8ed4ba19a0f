"""numpy restatement of the reference's map publishing and splat export -- TEST INFRASTRUCTURE ONLY.

FS = fl_ws/src/fl_slam_poc/fl_slam_poc.  JAX and ROS are not importable here, so the cited lines are
restated over the tile dicts of oracle.primitive_map (reference field names):
  * extract_primitive_map_view + its core       FS/backend/structures/primitive_map.py:501-577, :474-498
  * renderable_batch_from_view                  :580-616
  * PrimitiveMapPublisher.publish               FS/backend/map_publisher.py:131-242
  * _build_pointcloud2_from_view                :44-87 (the record bytes and the message's scalars)
  * the node's splat export loop                FS/backend/backend_node.py:2371-2459
jnp.argsort is stable (np.argsort(kind="stable") here; both order -0.0 == 0.0); jnp.linalg.solve / inv
are LAPACK LU on the CPU (np.linalg).  tests/test_map_export_host.py pins this file with known answers.
"""

from __future__ import annotations

import numpy as np

from oracle.primitive_map import GC_EPS_LIFT, GC_EPS_MASS, GC_VMF_N_LOBES, _solve, create_empty_tile  # noqa: F401


def extract_primitive_map_view(tile, tile_id=0, max_primitives=None, eps_lift=GC_EPS_LIFT, eps_mass=GC_EPS_MASS):
    """:501-577.  tile.count is the number of valid slots (the reference keeps it equal to the mask's sum)."""
    m = int(tile["Lambdas"].shape[0])
    count = int(np.asarray(tile["valid_mask"], bool).sum())
    if count == 0:                                                            # :522-535
        slots = np.zeros((0,), np.int32)
    else:
        slots = np.nonzero(np.asarray(tile["valid_mask"], bool))[0]           # :538 (jnp.where, size=count)
        if max_primitives is not None and count > max_primitives:             # :541-545
            top = np.argsort(-tile["weights"][slots], kind="stable")[:max_primitives]
            slots = slots[top]
    L = tile["Lambdas"][slots] + eps_lift * np.eye(3)[None]                   # :488
    es = np.sum(tile["etas"][slots], axis=1)                                  # :494
    kap = np.linalg.norm(es, axis=1) if len(slots) else np.zeros((0,))
    return dict(tile_id=int(tile_id), m_tile=m, slot_indices=slots.astype(np.int32),
                positions=_solve(L, tile["thetas"][slots]) if len(slots) else np.zeros((0, 3)),
                covariances=np.linalg.inv(L) if len(slots) else np.zeros((0, 3, 3)),
                directions=es / (kap[:, None] + eps_mass), kappas=kap, weights=tile["weights"][slots],
                primitive_ids=tile["primitive_ids"][slots], colors=tile["rgb"][slots], etas=tile["etas"][slots])


def renderable_batch_from_view(view, eps_lift=GC_EPS_LIFT):
    """:580-616."""
    S = np.asarray(view["covariances"], np.float64)
    Lw = np.linalg.inv(S + eps_lift * np.eye(3)[None]) if S.size else None
    return dict(mu_world=np.asarray(view["positions"], np.float64), Sigma_world=S, Lambda_world=Lw,
                eta=np.asarray(view["etas"], np.float64), mass=np.asarray(view["weights"], np.float64),
                color=np.asarray(view["colors"], np.float64), primitive_ids=np.asarray(view["primitive_ids"], np.int64))


def lexsort_order(primitive_ids, recency):
    """map_publisher.py:200: newest first, ties by primitive id, then by position (lexsort is stable)."""
    return np.lexsort((np.asarray(primitive_ids, np.int64), -np.asarray(recency, np.int64)))


def pointcloud2_bytes(positions, weights):
    """map_publisher.py:73-86: the packed records of _build_pointcloud2_from_view."""
    n = int(positions.shape[0])
    if n == 0:
        return b""
    dtype = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("intensity", "<f4")], align=False)
    arr = np.zeros((n,), dtype=dtype)
    with np.errstate(over="ignore", invalid="ignore"):
        arr["x"] = positions[:, 0].astype(np.float32)
        arr["y"] = positions[:, 1].astype(np.float32)
        arr["z"] = positions[:, 2].astype(np.float32)
        arr["intensity"] = np.clip(weights.astype(np.float32), 0.0, 1e6)
    return arr.tobytes()


def publish(tiles, tile_ids=None, max_primitives=None, eps_lift=GC_EPS_LIFT, eps_mass=GC_EPS_MASS, order=True):
    """map_publisher.py:131-242 over a dict tile_id -> tile.  Returns the published rows (with the rows'
    source tile ids and slots and the per-listed-tile row counts besides) and the record bytes.
    order=False leaves the rows in concatenation order (the export's order)."""
    if tile_ids is None:
        tile_ids = sorted(tiles)                                              # :143-144
    views, last, src_tile, tile_rows = [], [], [], []
    for tid in tile_ids:
        tile = tiles.get(int(tid))
        if tile is None:                                                      # :149-151
            tile_rows.append(0)
            continue
        v = extract_primitive_map_view(tile, tid, max_primitives, eps_lift, eps_mass)
        views.append(v)
        last.append(np.asarray(tile["last_supported_scan_seq"][v["slot_indices"]], np.int64))   # :161
        src_tile.append(np.full(len(v["slot_indices"]), int(tid), np.int64))
        tile_rows.append(len(v["slot_indices"]))
    cat = lambda k, shape: (np.concatenate([v[k] for v in views], axis=0) if views  # noqa: E731
                            else np.zeros(shape))
    out = dict(positions=cat("positions", (0, 3)), covariances=cat("covariances", (0, 3, 3)),
               directions=cat("directions", (0, 3)), kappas=cat("kappas", (0,)), weights=cat("weights", (0,)),
               etas=cat("etas", (0, GC_VMF_N_LOBES, 3)), colors=cat("colors", (0, 3)),
               primitive_ids=cat("primitive_ids", (0,)).astype(np.int64),
               slots=cat("slot_indices", (0,)).astype(np.int32),
               last_supported_scan_seq=np.concatenate(last) if last else np.zeros((0,), np.int64),
               tile_ids=np.concatenate(src_tile) if src_tile else np.zeros((0,), np.int64))
    n = int(out["positions"].shape[0])
    if order and n:
        o = lexsort_order(out["primitive_ids"], out["last_supported_scan_seq"])   # :198-205
        out = {k: v[o] for k, v in out.items()}
    out["Lambda_world"] = (np.linalg.inv(out["covariances"] + eps_lift * np.eye(3)[None])   # :232-233
                           if n else None)
    out["tile_rows"] = np.asarray(tile_rows, np.int32)
    out["n"] = n
    out["data"] = pointcloud2_bytes(out["positions"], out["weights"])
    out["cloud"] = dict(height=1, width=n, is_dense=True, is_bigendian=False, point_step=16, row_step=16 * n)
    return out


SPLAT_KEYS = ("positions", "covariances", "colors", "rgb", "weights", "directions", "kappas", "timestamps",
              "created_timestamps", "primitive_ids", "cam_mass", "lidar_mass", "rgb_cam_accum", "rgb_cam_denom", "n")


def export_splats(tiles, eps_lift=GC_EPS_LIFT, eps_mass=GC_EPS_MASS):
    """backend_node.py:2376-2456: the dict the node hands np.savez_compressed, or None where it skips."""
    parts = {k: [] for k in SPLAT_KEYS if k != "n"}
    for tid in sorted(tiles):                                                 # :2392
        tile = tiles[tid]
        v = extract_primitive_map_view(tile, tid, None, eps_lift, eps_mass)
        if len(v["slot_indices"]) == 0:                                       # :2394-2398
            continue
        s = v["slot_indices"].astype(np.int64)
        for k in ("positions", "covariances", "colors", "weights", "directions", "kappas", "primitive_ids"):
            parts[k].append(np.asarray(v[k]))
        parts["rgb"].append(np.asarray(tile["rgb"][s], np.float64))           # :2408-2414
        for k in ("timestamps", "created_timestamps", "cam_mass", "lidar_mass", "rgb_cam_accum", "rgb_cam_denom"):
            parts[k].append(np.asarray(tile[k][s], np.float64))
    if not parts["positions"]:                                                # :2416-2419
        return None
    out = {k: np.concatenate(v, axis=0) for k, v in parts.items()}
    out["n"] = int(out["positions"].shape[0])
    return {k: out[k] for k in SPLAT_KEYS}
