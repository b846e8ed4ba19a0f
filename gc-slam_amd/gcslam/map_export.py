"""Publishing and exporting the primitive map from the GPU: what the node does with the map after every
scan and at shutdown, with the reference's contracts, running gcs_pmap_export (libgcslam_hip.so):

  extract_primitive_map_view   FS/backend/structures/primitive_map.py:501-577 (the variable-length view of
                               one tile: valid slots in slot order, or the top max_primitives by weight)
  renderable_batch_from_view   :580-616
  publish_map                  FS/backend/map_publisher.py:131-242 (PrimitiveMapPublisher.publish: the views
                               of the listed tiles concatenated, newest first, as PointCloud2 bytes and a
                               RenderablePrimitiveBatch)
  export_splats                FS/backend/backend_node.py:2371-2459 (the shutdown .npz of every tile)
  export_rows                  the library call itself: any subset of the row fields, either order

Rows stay on the device as torch tensors; only the PointCloud2 bytes and the splat export come to the
host.  The views and batches also carry `directions`, `kappas` and an all-true `valid_mask`, so
gcslam.rendering.render_map_view takes them as they are.  There is no CPU fallback.
"""

from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _lib as L
from .primitive_map import GC_EPS_LIFT, GC_EPS_MASS, AtlasMap

ORDER_CONCAT = 0     # tile list order, then the per-tile order
ORDER_RECENCY = 1    # np.lexsort((primitive_id, -last_supported_scan_seq)), map_publisher.py:198-205
POINTFIELD_FLOAT32 = 7   # sensor_msgs/PointField.FLOAT32

# row field -> (element type, trailing shape; "B" is the lobe count)
_FIELDS = {
    "positions": ("f8", (3,)), "covariances": ("f8", (3, 3)), "directions": ("f8", (3,)), "kappas": ("f8", ()),
    "lambda_world": ("f8", (3, 3)), "weights": ("f8", ()), "etas": ("f8", ("B", 3)), "colors": ("f8", (3,)),
    "primitive_ids": ("i8", ()), "last_supported_scan_seq": ("i8", ()), "tile_ids": ("i8", ()), "slots": ("i4", ()),
    "timestamps": ("f8", ()), "created_timestamps": ("f8", ()), "cam_mass": ("f8", ()), "lidar_mass": ("f8", ()),
    "rgb_cam_accum": ("f8", (3,)), "rgb_cam_denom": ("f8", ()), "points": ("f4", (4,)),
}
ROW_FIELDS = tuple(_FIELDS)


def _torch():
    import torch
    return torch


class MapExportCapacityError(ValueError):
    """The rows exceed the capacity given; n_rows and tile_rows hold the counts to size the buffers by."""

    def __init__(self, msg, n_rows, tile_rows):
        super().__init__(msg)
        self.n_rows, self.tile_rows = int(n_rows), tile_rows


def export_buffers(n_lobes: int, capacity: int, dev: str, names: Sequence[str] = ROW_FIELDS):
    """Device arrays of `capacity` rows for the named fields (one allocation, 16-byte aligned segments) and
    the gcs_pmap_export_out naming them (a field not named stays NULL: the kernel skips it)."""
    torch = _torch()
    dt = {"f8": torch.float64, "i8": torch.int64, "i4": torch.int32, "f4": torch.float32}
    cap = int(capacity)
    shapes = {n: (cap,) + tuple(int(n_lobes) if s == "B" else s for s in _FIELDS[n][1]) for n in names}
    sizes = {n: int(np.prod(shapes[n])) * int(_FIELDS[n][0][1]) for n in names}
    buf = torch.empty(sum((z + 15) // 16 * 16 for z in sizes.values()), dtype=torch.uint8, device=dev)
    t, off = {}, 0
    for n in names:
        t[n] = buf[off:off + sizes[n]].view(dt[_FIELDS[n][0]]).view(shapes[n])
        off += (sizes[n] + 15) // 16 * 16
    o = L.GcsPmapExportOut()
    for n, x in t.items():
        setattr(o, n, x.data_ptr() if cap else None)
    return t, o, buf


@dataclass
class MapExportRows:
    """gcs_pmap_export's result: `rows[name]` are device tensors of n_rows rows in the order asked for."""
    rows: Dict[str, object]
    n_rows: int
    tile_rows: np.ndarray        # rows per listed tile (0 for a tile the map lacks)
    tile_ids: List[int]
    order: int


def export_rows(atlas_map: AtlasMap, tile_ids: Optional[Sequence[int]] = None, max_primitives: Optional[int] = None,
                order: int = ORDER_CONCAT, eps_lift: float = GC_EPS_LIFT, eps_mass: float = GC_EPS_MASS,
                fields: Sequence[str] = ROW_FIELDS, capacity: Optional[int] = None) -> MapExportRows:
    """The listed tiles' variable-length views as one row set (tile_ids None: every tile, sorted ids).  A
    tile the map lacks is skipped, an id listed twice contributes twice.  `capacity`: rows to allocate; by
    default the map's bookkeeping sizes the buffers and the call is repeated if the device counts more
    (with a capacity given, more rows raise MapExportCapacityError)."""
    if max_primitives is not None and int(max_primitives) < 0:
        raise ValueError(f"max_primitives must be >= 0, got {max_primitives}")
    ids = sorted(atlas_map.tile_ids) if tile_ids is None else [int(t) for t in tile_ids]
    n = len(ids)
    dev = f"cuda:{atlas_map.device}"
    # max_primitives = 0 keeps no row of a non-empty tile (argsort(...)[:0]); the library's 0 means "no limit"
    if max_primitives is not None and int(max_primitives) == 0:
        t, _, _ = export_buffers(atlas_map.n_lobes, 0, dev, fields)
        return MapExportRows(t, 0, np.zeros(n, np.int32), ids, int(order))
    maxp = 0 if max_primitives is None else int(max_primitives)
    idx = np.ascontiguousarray(np.array([atlas_map.index(t, create=False) for t in ids], dtype=np.int32))
    tids = np.ascontiguousarray(np.array(ids, dtype=np.int64))
    if capacity is None:
        per = [min(atlas_map.counts.get(t, atlas_map.m_tile), maxp or atlas_map.m_tile)
               for t, i in zip(ids, idx) if i >= 0]
        cap = int(sum(per))
    else:
        cap = int(capacity)
    n_rows = np.zeros(1, np.int32)
    tile_rows = np.zeros(max(n, 1), np.int32)
    atlas_map._stream()
    while True:
        t, o, _ = export_buffers(atlas_map.n_lobes, cap, dev, fields)
        rc = atlas_map.lib.gcs_pmap_export(atlas_map.h, L.iptr(idx), tids.ctypes.data_as(L.c_int64_p), n, maxp,
                                           int(order), float(eps_lift), float(eps_mass), cap, C.byref(o),
                                           L.iptr(n_rows), L.iptr(tile_rows))
        if rc == -1 and int(n_rows[0]) > cap:
            if capacity is not None:
                msg = atlas_map.lib.gcs_pmap_last_error(atlas_map.h).decode(errors="replace")
                raise MapExportCapacityError(f"gcs_pmap_export: {msg}: {int(n_rows[0])} rows, capacity {cap}",
                                             n_rows[0], tile_rows[:n].copy())
            cap = int(n_rows[0])     # the bookkeeping was behind the device: size by its count
            continue
        atlas_map._chk(rc, "gcs_pmap_export")
        break
    nr = int(n_rows[0])
    return MapExportRows({k: v[:nr] for k, v in t.items()}, nr, tile_rows[:n].copy(), ids, int(order))


# ---------------------------------------------------------------------- the reference's dataclasses
@dataclass
class PrimitiveMapView:
    """primitive_map.py:236-267 (device tensors), with what render_map_view reads besides."""
    tile_id: int
    m_tile: int
    slot_indices: object     # (N,) int32
    positions: object        # (N, 3)
    covariances: object      # (N, 3, 3)
    directions: object       # (N, 3)
    kappas: object           # (N,)
    weights: object          # (N,)
    primitive_ids: object    # (N,) int64
    colors: object = None    # (N, 3) (the tile's rgb)
    etas: object = None      # (N, B, 3)
    valid_mask: object = None                # (N,) bool, all true
    last_supported_scan_seq: object = None   # (N,) int64
    lambda_world: object = None              # (N, 3, 3): inv(covariances + eps_lift I), from the same kernel
    eps_lift: float = GC_EPS_LIFT

    @property
    def count(self) -> int:
        return int(self.positions.shape[0])


@dataclass
class RenderablePrimitiveBatch:
    """primitive_map.py:453-471 (device tensors).  Lambda_world is None for an empty batch, as the
    reference leaves it."""
    mu_world: object
    Sigma_world: object
    Lambda_world: object
    eta: object
    mass: object
    color: object
    primitive_ids: object = None
    directions: object = None
    kappas: object = None
    valid_mask: object = None
    last_supported_scan_seq: object = None
    source_tile_ids: object = None     # (N,) int64: the tile each row came from
    source_slots: object = None        # (N,) int32: ... and its slot

    # the names gcslam.rendering.render_map_view reads
    @property
    def positions(self):
        return self.mu_world

    @property
    def covariances(self):
        return self.Sigma_world

    @property
    def colors(self):
        return self.color

    @property
    def count(self) -> int:
        return int(self.mu_world.shape[0])


@dataclass
class PointField:
    name: str
    offset: int
    datatype: int = POINTFIELD_FLOAT32
    count: int = 1


def _cloud_fields():
    return [PointField("x", 0), PointField("y", 4), PointField("z", 8), PointField("intensity", 12)]


@dataclass
class PointCloud2Data:
    """What a sensor_msgs/PointCloud2 needs (map_publisher.py:44-87); the header is the node's."""
    data: bytes = b""
    width: int = 0
    height: int = 1
    point_step: int = 16
    row_step: int = 0
    is_dense: bool = True
    is_bigendian: bool = False
    fields: List[PointField] = field(default_factory=_cloud_fields)


_VIEW_FIELDS = ("positions", "covariances", "directions", "kappas", "lambda_world", "weights", "etas", "colors",
                "primitive_ids", "last_supported_scan_seq", "slots")
_BATCH_FIELDS = _VIEW_FIELDS + ("tile_ids", "points")


def _all_true(n, dev):
    torch = _torch()
    return torch.ones(n, dtype=torch.bool, device=dev)


def extract_primitive_map_view(atlas_map: AtlasMap, tile_id: int, max_primitives: Optional[int] = None,
                               eps_lift: float = GC_EPS_LIFT, eps_mass: float = GC_EPS_MASS) -> PrimitiveMapView:
    """:501-577: the tile's valid slots in slot order; with more than max_primitives of them, the first
    max_primitives of the stable order of -weight.  An empty or absent tile gives the zero-length view."""
    r = export_rows(atlas_map, [int(tile_id)], max_primitives, ORDER_CONCAT, eps_lift, eps_mass, _VIEW_FIELDS)
    x = r.rows
    return PrimitiveMapView(tile_id=int(tile_id), m_tile=atlas_map.m_tile, slot_indices=x["slots"],
                            positions=x["positions"], covariances=x["covariances"], directions=x["directions"],
                            kappas=x["kappas"], weights=x["weights"], primitive_ids=x["primitive_ids"],
                            colors=x["colors"], etas=x["etas"],
                            valid_mask=_all_true(r.n_rows, x["positions"].device),
                            last_supported_scan_seq=x["last_supported_scan_seq"], lambda_world=x["lambda_world"],
                            eps_lift=float(eps_lift))


def renderable_batch_from_view(view: PrimitiveMapView, eps_lift: float = GC_EPS_LIFT) -> RenderablePrimitiveBatch:
    """:580-616.  Lambda_world = inv(Sigma + eps_lift I) was computed with the view (the same kernel, the
    view's eps_lift): a different eps_lift here is refused rather than recomputed off the kernel."""
    if float(eps_lift) != float(view.eps_lift):
        raise ValueError(f"renderable_batch_from_view: the view was extracted with eps_lift={view.eps_lift}; "
                         f"extract it with eps_lift={eps_lift}")
    return RenderablePrimitiveBatch(mu_world=view.positions, Sigma_world=view.covariances,
                                    Lambda_world=view.lambda_world if view.count else None, eta=view.etas,
                                    mass=view.weights, color=view.colors, primitive_ids=view.primitive_ids,
                                    directions=view.directions, kappas=view.kappas, valid_mask=view.valid_mask,
                                    last_supported_scan_seq=view.last_supported_scan_seq)


def publish_map(atlas_map: AtlasMap, tile_ids: Optional[Sequence[int]] = None, max_primitives: Optional[int] = None,
                eps_lift: float = GC_EPS_LIFT, eps_mass: float = GC_EPS_MASS, order: int = ORDER_RECENCY):
    """map_publisher.py:131-242: (cloud, batch) of the listed tiles (None: all, sorted ids), newest first
    with ties by primitive id (order=ORDER_CONCAT: as concatenated).  cloud.data are the packed x, y, z,
    intensity records; the batch holds the same rows, in the same order, on the device."""
    r = export_rows(atlas_map, tile_ids, max_primitives, order, eps_lift, eps_mass, _BATCH_FIELDS)
    x, n = r.rows, r.n_rows
    data = x["points"].cpu().numpy().tobytes() if n else b""
    cloud = PointCloud2Data(data=data, width=n, row_step=16 * n)
    batch = RenderablePrimitiveBatch(mu_world=x["positions"], Sigma_world=x["covariances"],
                                     Lambda_world=x["lambda_world"] if n else None, eta=x["etas"], mass=x["weights"],
                                     color=x["colors"], primitive_ids=x["primitive_ids"], directions=x["directions"],
                                     kappas=x["kappas"], valid_mask=_all_true(n, x["positions"].device),
                                     last_supported_scan_seq=x["last_supported_scan_seq"],
                                     source_tile_ids=x["tile_ids"], source_slots=x["slots"])
    return cloud, batch


_SPLAT_FIELDS = ("positions", "covariances", "colors", "weights", "directions", "kappas", "timestamps",
                 "created_timestamps", "primitive_ids", "cam_mass", "lidar_mass", "rgb_cam_accum", "rgb_cam_denom")
SPLAT_KEYS = ("positions", "covariances", "colors", "rgb", "weights", "directions", "kappas", "timestamps",
              "created_timestamps", "primitive_ids", "cam_mass", "lidar_mass", "rgb_cam_accum", "rgb_cam_denom", "n")


def export_splats(atlas_map: AtlasMap, path: Optional[str] = None, eps_lift: float = GC_EPS_LIFT,
                  eps_mass: float = GC_EPS_MASS) -> Optional[dict]:
    """backend_node.py:2371-2459: every tile's full view in sorted tile-id order, with the slot-local
    fields, as the dict of arrays the node saves (keys SPLAT_KEYS); written with np.savez_compressed when
    `path` is given.  None, and nothing written, when the map has no valid primitive."""
    r = export_rows(atlas_map, None, None, ORDER_CONCAT, eps_lift, eps_mass, _SPLAT_FIELDS)
    if r.n_rows == 0:
        return None
    out = {k: r.rows[k].cpu().numpy() for k in _SPLAT_FIELDS}
    out["rgb"] = out["colors"].copy()      # both are the tile's rgb at the view's slots (:553, :2408)
    out["n"] = int(r.n_rows)
    out = {k: out[k] for k in SPLAT_KEYS}
    if path:
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        np.savez_compressed(path, **out)
    return out
