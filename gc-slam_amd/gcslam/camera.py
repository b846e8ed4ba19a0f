"""The camera half of the live primitive path's measurement batch on the MI355X: what the reference's
node does per scan between its visual feature buffer and feature_list_to_camera_batch
(FS/backend/backend_node.py:1865-1925) -- LiDAR-camera depth fusion along each feature's pixel ray
(FS/frontend/sensors/lidar_camera_depth_fusion.py), the fused splat (splat_prep.py), the move to the
base frame and the camera slice of the MeasurementBatch (camera_batch_utils.py,
structures/measurement_batch.py:165-259) -- through gcs_camera_splats (libgcslam_hip.so).  The batch
it returns goes to extract_lidar_surfels(base_batch=...) or to
process_scan_single_hypothesis(camera_batch=..., config.camera_batch_policy="use").  A CameraFrame (the
features with the camera's intrinsics and pose) goes to process_scan_single_hypothesis in the batch's
place: the slice is then built from the scan's own points inside the one-call live scan
(gcs_live_scan_camera)."""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field, fields
from typing import Optional

import numpy as np

from . import _lib as L
from .surfels import GC_N_FEAT, GC_N_SURFEL, MeasurementBatch, create_empty_measurement_batch

GC_EPS_LIFT = 1e-9   # constants.py:71


@dataclass(frozen=True)
class DepthFusionConfig:
    """LidarCameraDepthFusionConfig (lidar_camera_depth_fusion.py:29-63): same fields and defaults."""
    depth_fusion_weight_camera: float = 1.0
    depth_fusion_weight_lidar: float = 1.0
    gamma_lidar: float = 1.0
    lidar_projection_radius_pix: float = 3.0
    lidar_plane_fit_min_points: int = 3
    lidar_depth_base_sigma_m: float = 0.02
    lidar_incidence_sigma_scale: float = 1.0
    depth_var_min_m2: float = 1e-8
    point_support_n0: float = 3.0
    point_support_alpha: float = 1.0
    spread_mad_beta: float = 10.0
    repr_gamma: float = 10.0
    lidar_ray_plane_fit_max_points: int = 64
    plane_intersection_delta: float = 1e-6
    plane_angle_sigmoid_alpha: float = 10.0
    plane_angle_sigmoid_t: float = 0.1
    plane_planarity_sigmoid_beta: float = 5.0
    plane_planarity_rho0: float = 0.3
    plane_residual_exp_gamma: float = 100.0
    plane_fit_eps: float = 1e-12
    depth_min_m: float = 0.05
    depth_sigma_max_sq: float = 1e4
    depth_min_sigmoid_alpha_z: float = 20.0


@dataclass(frozen=True)
class PinholeIntrinsics:
    """visual_types.py:16-21."""
    fx: float
    fy: float
    cx: float
    cy: float


_FEATURE_ARRAYS = (("u", 0), ("v", 0), ("depth_Lambda_c", 0), ("depth_theta_c", 0), ("xyz", 3), ("cov", 9),
                   ("weight", 0), ("kappa_app", 0), ("mu_app", 3), ("color", 3))


def _torch():
    import torch
    return torch


def feature_arrays(features) -> dict:
    """Host arrays of a feature set.  features: a dict of arrays (u, v, xyz (M,3), cov (M,3,3), weight,
    kappa_app and optionally depth_Lambda_c, depth_theta_c, mu_app + has_mu, color + has_color), or a
    sequence of objects with Feature3D's attributes (visual_types.py:24-61: u, v, xyz, cov_xyz, weight,
    meta, mu_app, kappa_app, color); meta["depth_Lambda_c"] / meta["depth_theta_c"] default to 0
    (splat_prep.py:74-75)."""
    if isinstance(features, dict):
        m = int(np.asarray(features["u"]).reshape(-1).shape[0])
        out = {}
        for name, w in _FEATURE_ARRAYS:
            if name in features:
                out[name] = np.ascontiguousarray(features[name], np.float64).reshape((m, w) if w else (m,))
            elif name in ("depth_Lambda_c", "depth_theta_c", "mu_app", "color"):
                out[name] = np.zeros((m, w) if w else (m,))
            else:
                raise KeyError(f"features: missing array {name!r}")
        for flag, name in (("has_mu", "mu_app"), ("has_color", "color")):
            present = np.full(m, name in features, bool)
            out[flag] = np.ascontiguousarray(features.get(flag, present)).astype(np.uint8).reshape(m)
        return out
    feats = list(features)
    m = len(feats)
    out = {name: np.zeros((m, w) if w else (m,)) for name, w in _FEATURE_ARRAYS}
    out["has_mu"], out["has_color"] = np.zeros(m, np.uint8), np.zeros(m, np.uint8)
    for i, f in enumerate(feats):
        meta = getattr(f, "meta", None) or {}
        out["u"][i], out["v"][i] = float(f.u), float(f.v)
        out["depth_Lambda_c"][i] = float(meta.get("depth_Lambda_c", 0.0))
        out["depth_theta_c"][i] = float(meta.get("depth_theta_c", 0.0))
        out["xyz"][i] = np.asarray(f.xyz, np.float64).reshape(3)
        out["cov"][i] = np.asarray(f.cov_xyz, np.float64).reshape(9)
        out["weight"][i], out["kappa_app"][i] = float(f.weight), float(getattr(f, "kappa_app", 0.0))
        mu = getattr(f, "mu_app", None)
        if mu is not None:
            out["mu_app"][i], out["has_mu"][i] = np.asarray(mu, np.float64).reshape(3), 1
        c = getattr(f, "color", None)
        if c is not None and np.size(c) >= 3:   # camera_batch_utils.py:50-54
            out["color"][i], out["has_color"][i] = np.asarray(c, np.float64).ravel()[:3], 1
    return out


class CameraSplatBuilder:
    """A gcs_camsplat_ctx: workspace for up to max_points LiDAR points on one GPU."""

    def __init__(self, config: Optional[DepthFusionConfig] = None, n_feat: int = GC_N_FEAT,
                 n_surfel: int = GC_N_SURFEL, eps_lift: float = GC_EPS_LIFT, pixel_sigma: float = 1.0,
                 max_points: int = 65536, max_candidates: int = 1024, device: int = 0):
        self.config = config or DepthFusionConfig()
        self.lib = L.load()
        c = L.GcsCamsplatConfig()
        L.check(self.lib.gcs_camsplat_config_defaults(C.byref(c)), None, "gcs_camsplat_config_defaults")
        for f in fields(self.config):
            setattr(c, f.name, getattr(self.config, f.name))
        c.pixel_sigma, c.eps_lift = float(pixel_sigma), float(eps_lift)
        c.n_feat, c.n_surfel = int(n_feat), int(n_surfel)
        c.max_points, c.max_candidates, c.device = int(max_points), int(max_candidates), int(device)
        h = C.c_void_p()
        rc = self.lib.gcs_camsplat_ctx_create(C.byref(c), C.byref(h))
        if rc != 0:
            raise (ValueError if rc == -1 else RuntimeError)(f"gcs_camsplat_ctx_create failed ({rc})")
        self.h = h
        self.n_feat, self.n_surfel = int(n_feat), int(n_surfel)
        self.device, self.max_points = int(device), int(max_points)

    def close(self):
        if getattr(self, "h", None):
            self.lib.gcs_camsplat_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc != 0:
            msg = self.lib.gcs_camsplat_last_error(self.h).decode(errors="replace")
            raise (ValueError if rc in (-1, -3) else RuntimeError)(f"{what} failed ({rc}): {msg}")

    def build(self, features, points_base, intrinsics: PinholeIntrinsics, R_base_camera, t_base_camera,
              timestamp_sec: float, want_diag: bool = False) -> MeasurementBatch:
        """The camera batch of one scan (LiDAR slice empty).  features: see feature_arrays (host arrays,
        or a dict of device tensors prepared by device_features); points_base: (N, 3) f64, host or
        device.  want_diag: batch.camera_diag holds the per-feature diagnostics (device tensors).  A
        feature with more than max_candidates points within its radius raises RuntimeError naming it."""
        torch = _torch()
        dev = f"cuda:{self.device}"
        fa = features if getattr(features, "_on_device", False) else self.device_features(features)
        if int(fa["u"].shape[0]) == 0:   # camera_batch_utils.py:35-37
            return create_empty_measurement_batch(self.n_feat, self.n_surfel, dev)
        p = torch.as_tensor(points_base, dtype=torch.float64, device=dev).reshape(-1, 3).contiguous()
        return self._run(fa, p, None, intrinsics, R_base_camera, t_base_camera, timestamp_sec, want_diag)

    def build_from_records(self, features, xyz_dev, point_step: int, xyz_format: int, n_points: int,
                           intrinsics: PinholeIntrinsics, R_base_camera, t_base_camera, timestamp_sec: float,
                           want_diag: bool = False) -> MeasurementBatch:
        """build() on the scan's own records (gcs_camera_splats_scan): xyz_dev, a device tensor holding
        n_points records of point_step bytes -- xyz_format 0: float32 x, y, z at bytes 0, 4, 8 (what
        gcs_scan_inputs.xyz_dev holds); 1: float64 at bytes 0, 8, 16.  Bit for bit build() on the float64
        array of the same values."""
        dev = f"cuda:{self.device}"
        fa = features if getattr(features, "_on_device", False) else self.device_features(features)
        if int(fa["u"].shape[0]) == 0:
            return create_empty_measurement_batch(self.n_feat, self.n_surfel, dev)
        need = (int(n_points) - 1) * int(point_step) + (24 if int(xyz_format) == 1 else 12) if n_points > 0 else 0
        if n_points < 0 or need > xyz_dev.numel() * xyz_dev.element_size():
            raise ValueError("xyz_dev holds fewer than n_points records")
        return self._run(fa, xyz_dev, (int(point_step), int(xyz_format), int(n_points)), intrinsics, R_base_camera,
                         t_base_camera, timestamp_sec, want_diag)

    def inputs_struct(self, fa, intrinsics, R_base_camera, t_base_camera, timestamp_sec) -> "L.GcsCamsplatInputs":
        """gcs_camsplat_inputs of device features fa (points_base / n_points left unset)."""
        i = L.GcsCamsplatInputs()
        R = np.ascontiguousarray(R_base_camera, np.float64).reshape(9)
        t = np.ascontiguousarray(t_base_camera, np.float64).reshape(3)
        i.R_base_camera[:], i.t_base_camera[:] = R.tolist(), t.tolist()
        i.fx, i.fy, i.cx, i.cy = (float(getattr(intrinsics, k)) for k in ("fx", "fy", "cx", "cy"))
        i.n_features = int(fa["u"].shape[0])
        for name in ("u", "v", "depth_Lambda_c", "depth_theta_c", "xyz", "cov", "weight", "kappa_app", "mu_app",
                     "has_mu", "color", "has_color"):
            setattr(i, name, fa[name].data_ptr())
        i.timestamp_sec = float(timestamp_sec)
        return i

    def diag_tensors(self, m: int) -> dict:
        """Fresh per-feature diagnostic arrays (gcs_camsplat_outputs' optional pointers) for m features."""
        torch = _torch()
        dt = {"n_pt": torch.int32, "fused": torch.uint8}
        return {k: torch.empty(m, dtype=dt.get(k, torch.float64), device=f"cuda:{self.device}")
                for k in L.CAMSPLAT_DIAG_FIELDS}

    def _run(self, fa, points, records, intrinsics, R_base_camera, t_base_camera, timestamp_sec, want_diag):
        torch = _torch()
        dev = f"cuda:{self.device}"
        batch = create_empty_measurement_batch(self.n_feat, self.n_surfel, dev)
        i = self.inputs_struct(fa, intrinsics, R_base_camera, t_base_camera, timestamp_sec)
        o = L.GcsCamsplatOutputs()
        sl = slice(0, self.n_feat)
        for name in L.CAMSPLAT_BATCH_FIELDS:
            x = getattr(batch, name)[sl]
            setattr(o, name, (x.view(torch.uint8) if name == "valid_mask" else x).data_ptr())
        diag = None
        if want_diag:
            diag = self.diag_tensors(int(i.n_features))
            for k, x in diag.items():
                setattr(o, k, x.data_ptr())
        ts = torch.cuda.current_stream(dev)
        self._chk(self.lib.gcs_camsplat_ctx_set_stream(self.h, C.c_void_p(ts.cuda_stream)), "gcs_camsplat_ctx_set_stream")
        if not ts.cuda_stream:
            # torch's default stream is handle 0, for which the context queues on a stream of its own that the
            # default stream does not order: what produced the features and points there (an upload, or
            # gcs_visual_features, which does not wait) has to be complete first
            ts.synchronize()
        if records is None:
            i.points_base, i.n_points = points.data_ptr(), int(points.shape[0])
            self._chk(self.lib.gcs_camera_splats(self.h, C.byref(i), C.byref(o)), "gcs_camera_splats")
        else:
            step, fmt, n = records
            self._chk(self.lib.gcs_camera_splats_scan(self.h, C.byref(i), C.c_void_p(points.data_ptr()), step, fmt, n,
                                                      C.byref(o)), "gcs_camera_splats_scan")
        batch.n_camera_valid = int(o.n_camera_valid)
        if diag is not None:
            batch.camera_diag = diag
        return batch

    def device_features(self, features) -> dict:
        """feature_arrays(features) on the builder's GPU (reusable across calls on the same features): the
        twelve arrays through one pinned staging buffer and one H2D copy, as the scan's points go."""
        return _upload_features(feature_arrays(features), self.device)


class _DeviceFeatures(dict):
    _on_device = True


_stage = {}


def _upload_features(fa: dict, device: int) -> "_DeviceFeatures":
    """Host feature arrays (feature_arrays' dict) -> device tensors: one pinned staging buffer per
    (device, stream), grown to the largest feature set seen, and one H2D copy into a fresh device buffer
    (the f64 arrays first, 8-byte aligned, then the two uint8 flags); before the staging buffer is refilled
    the event of its previous copy is waited on."""
    torch = _torch()
    dev = f"cuda:{device}"
    m = int(fa["u"].shape[0])
    widths = [(name, max(w, 1)) for name, w in _FEATURE_ARRAYS]
    nbytes = (8 * m * sum(w for _, w in widths) + 2 * m + 7) // 8 * 8
    stream = torch.cuda.current_stream(dev)
    key = (int(device), stream.cuda_stream)
    ent = _stage.get(key)
    if ent is not None and ent[0].numel() < nbytes:
        if ent[2]:
            ent[1].synchronize()   # the last copy out of the old buffer before it is dropped
        ent = None
    if ent is None:
        hb = torch.empty(-(-max(nbytes, 1 << 16) // 4096) * 4096, dtype=torch.uint8).pin_memory()
        ent = _stage[key] = [hb, torch.cuda.Event(), False, hb.numpy()]
    hb, ev, used, hn = ent
    if used:
        ev.synchronize()
    off, spans = 0, []
    for name, w in widths:
        z = 8 * m * w
        hn[off:off + z].view(np.float64)[...] = np.asarray(fa[name], np.float64).reshape(-1)
        spans.append((name, off, z, torch.float64, (m, w) if w > 1 else (m,)))
        off += z
    for name in ("has_mu", "has_color"):
        hn[off:off + m] = np.asarray(fa[name]).astype(np.uint8).reshape(-1)
        spans.append((name, off, m, torch.uint8, (m,)))
        off += m
    d = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    if nbytes:
        d.copy_(hb[:nbytes], non_blocking=True)
        ev.record(stream)
        ent[2] = True
    return _DeviceFeatures((name, d[o:o + z].view(dt).view(sh)) for name, o, z, dt, sh in spans)


_builders = {}


def _builder_for(config, n_feat, n_surfel, eps_lift, n_points, device, max_candidates=1024):
    key = (config, int(n_feat), int(n_surfel), float(eps_lift), int(device), int(max_candidates))
    b = _builders.get(key)
    if b is None or b.h is None or b.max_points < n_points:
        if b is not None:
            b.close()
        b = _builders[key] = CameraSplatBuilder(config, n_feat=n_feat, n_surfel=n_surfel, eps_lift=eps_lift,
                                                max_points=max(n_points, 8192), max_candidates=max_candidates,
                                                device=device)
    return b


@dataclass
class CameraFrame:
    """One scan's visual features as the node holds them ahead of its hypothesis loop
    (backend_node.py:1834-1925): the feature set (see feature_arrays; or device features, as
    CameraSplatBuilder.device_features and gcslam.visual.extract_visual_features return them, which are
    used where they are with no host copy), the pinhole intrinsics, the camera's
    pose in the base frame (p_base = R p_camera + t), the batch's timestamp and the depth-fusion config.
    process_scan_single_hypothesis(camera_batch=CameraFrame(...), camera_batch_policy="use") builds the
    batch's camera slice from the scan's own points inside the scan (the node's splat_prep_fused reads the
    scan's base-frame points, :1872-1884).  want_diag: result.camera_diag holds the per-feature
    diagnostics.  max_candidates: the points within one feature's radius held at once (<= 1024); a denser
    feature fails the scan, naming the feature."""
    features: object
    intrinsics: PinholeIntrinsics
    R_base_camera: object
    t_base_camera: object
    timestamp_sec: float
    config: DepthFusionConfig = field(default_factory=DepthFusionConfig)
    want_diag: bool = False
    max_candidates: int = 1024

    def __post_init__(self):
        if self.config is None:
            self.config = DepthFusionConfig()
        if not isinstance(self.config, DepthFusionConfig):
            raise TypeError("CameraFrame.config: a DepthFusionConfig")
        R = np.array(self.R_base_camera, np.float64)
        t = np.array(self.t_base_camera, np.float64)
        if R.shape != (3, 3) or not np.isfinite(R).all():
            raise ValueError("CameraFrame.R_base_camera: a finite 3 x 3 matrix")
        if t.reshape(-1).shape != (3,) or not np.isfinite(t).all():
            raise ValueError("CameraFrame.t_base_camera: three finite values")
        self.R_base_camera, self.t_base_camera = R, t.reshape(3)
        k = [float(getattr(self.intrinsics, n)) for n in ("fx", "fy", "cx", "cy")]
        if not np.isfinite(k).all() or k[0] <= 0.0 or k[1] <= 0.0:
            raise ValueError("CameraFrame.intrinsics: finite fx, fy > 0, cx, cy")
        self.timestamp_sec = float(self.timestamp_sec)
        if not np.isfinite(self.timestamp_sec):
            raise ValueError("CameraFrame.timestamp_sec is not finite")
        if not 1 <= int(self.max_candidates) <= 1024:
            raise ValueError("CameraFrame.max_candidates outside [1, 1024]")
        # host arrays, validated once -- or device features (CameraSplatBuilder.device_features,
        # gcslam.visual.extract_visual_features), which stay where they are: arrays is then None
        on_device = getattr(self.features, "_on_device", False)
        self.device_arrays = self.features if on_device else None
        self.arrays = None if on_device else feature_arrays(self.features)
        held = self.device_arrays if on_device else self.arrays
        m = self.n_features
        if m > 65535:
            raise ValueError("CameraFrame: more than 65535 features")
        for name, w in _FEATURE_ARRAYS + ((("has_mu", 0), ("has_color", 0)) if on_device else ()):
            if name not in held:
                raise KeyError(f"features: missing array {name!r}")
            if tuple(held[name].shape) != ((m, w) if w else (m,)):
                raise ValueError(f"CameraFrame.features[{name!r}]: shape {tuple(held[name].shape)}")
        if on_device:
            torch = _torch()
            for name, w in _FEATURE_ARRAYS + (("has_mu", 0), ("has_color", 0)):
                x, dt = held[name], (torch.uint8 if name.startswith("has_") else torch.float64)
                if not (torch.is_tensor(x) and x.is_cuda and x.dtype == dt and x.is_contiguous()):
                    raise ValueError(f"CameraFrame.features[{name!r}]: a contiguous {dt} device tensor")

    @property
    def n_features(self) -> int:
        return int((self.arrays if self.arrays is not None else self.device_arrays)["u"].shape[0])

    def features_on(self, device: int) -> "_DeviceFeatures":
        """The features on GPU `device`: the frame's own device tensors, or its host arrays uploaded."""
        if self.device_arrays is None:
            return _upload_features(self.arrays, device)
        if self.n_features and self.device_arrays["u"].device.index != int(device):
            raise ValueError(f"CameraFrame: device features on {self.device_arrays['u'].device}, the scan on "
                             f"cuda:{int(device)}")
        return self.device_arrays

    @property
    def n_valid(self) -> int:   # (an empty frame is no camera batch: the scan runs LiDAR-only)
        return self.n_features

    def builder(self, n_feat, n_surfel, eps_lift, n_points, device) -> CameraSplatBuilder:
        return _builder_for(self.config, n_feat, n_surfel, eps_lift, n_points, device, self.max_candidates)


def camera_batch_from_features(features, points_base, intrinsics: PinholeIntrinsics, R_base_camera, t_base_camera,
                               timestamp_sec: float, config: Optional[DepthFusionConfig] = None,
                               n_feat: int = GC_N_FEAT, n_surfel: int = GC_N_SURFEL, eps_lift: float = GC_EPS_LIFT,
                               device: int = 0, want_diag: bool = False) -> MeasurementBatch:
    """backend_node.py:1865-1925 for one scan: splat_prep_fused on the scan's base-frame points, the
    base-frame conversion and feature_list_to_camera_batch.  Returns a MeasurementBatch whose camera
    slice holds the first min(M, n_feat) features; an empty feature list gives
    create_empty_measurement_batch."""
    n_points = int(points_base.shape[0]) if hasattr(points_base, "shape") else len(points_base)
    b = _builder_for(config or DepthFusionConfig(), n_feat, n_surfel, eps_lift, n_points, device)
    return b.build(features, points_base, intrinsics, R_base_camera, t_base_camera, timestamp_sec,
                   want_diag=want_diag)
