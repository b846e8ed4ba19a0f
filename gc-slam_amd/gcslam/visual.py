"""Visual features from an RGB-D frame and a keypoint list on the MI355X: what the reference's
visual_feature_node does per frame after ORB (src/visual_feature_node.cpp:493-652 -- the robust depth
sample, the Student-t effective variance, the quadratic surface fit, the back-projection with its
closed-form covariance, the medial-axis inflation, the vMF kappa, weights and colour) and what
_feature_batch_to_list (FS/backend/backend_node.py:1589-1650) makes of the message rows, through
gcs_visual_features (libgcslam_hip.so).  The result is the device feature dict of gcslam.camera: it goes
to CameraSplatBuilder.build or, in a CameraFrame, to process_scan_single_hypothesis, with no host copy.
Keypoints are (u, v, response) rows, cv::KeyPoint's pt.x, pt.y and response: the caller's, from any
detector, or with keypoints=None the library's own (gcslam.keypoints: FAST-9, Harris response, stable top-N
at pyramid level 0, no parity with cv::ORB), detected from rgb on the same stream and passed device to
device."""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, fields
from typing import Optional, Union

import numpy as np

from . import _lib as L
from .camera import CameraFrame, DepthFusionConfig, PinholeIntrinsics, _DeviceFeatures
from .keypoints import (GridConfig, KeypointConfig, PyramidConfig, detect_keypoints, detect_keypoints_grid,
                        detect_keypoints_pyramid)

_MODES = {"nearest": L.VF_NEAREST, "median3": L.VF_MEDIAN3, "median5": L.VF_MEDIAN5, "hex": L.VF_HEX}
_MODELS = {"linear": L.VF_DEPTH_LINEAR, "quadratic": L.VF_DEPTH_QUADRATIC}


@dataclass(frozen=True)
class VisualFeatureConfig:
    """The node's declared parameters (visual_feature_node.cpp:70-103): same names and defaults.
    max_keypoints: the most keypoints one call takes (the context's capacity)."""
    max_features: int = 512
    depth_sample_mode: str = "median3"
    pixel_sigma: float = 1.0
    depth_model: str = "linear"
    depth_sigma0: float = 0.01
    depth_sigma_slope: float = 0.01
    min_depth_m: float = 0.05
    max_depth_m: float = 80.0
    depth_validity_slope: float = 5.0
    response_soft_scale: float = 50.0
    depth_scale: float = 1.0
    cov_reg_eps: float = 1e-9
    invalid_cov_inflate: float = 1e6
    hex_radius: int = 2
    quad_fit_radius: int = 2
    quad_fit_min_points: int = 6
    quad_fit_lstsq_eps: float = 1e-8
    student_t_nu: float = 3.0
    student_t_w_min: float = 0.1
    ma_tau: float = 10.0
    ma_delta_inflate: float = 1e-4
    kappa0: float = 1.0
    kappa_alpha: float = 10.0
    kappa_max: float = 100.0
    kappa_min: float = 0.1
    max_keypoints: int = 4096


def config_struct(config: Optional[VisualFeatureConfig] = None, device: int = 0) -> "L.GcsVisfeatConfig":
    """gcs_visfeat_config of a VisualFeatureConfig."""
    config = config or VisualFeatureConfig()
    if config.depth_sample_mode not in _MODES:
        raise ValueError(f"Unknown depth_sample_mode: {config.depth_sample_mode}")   # :256
    if config.depth_model not in _MODELS:
        raise ValueError(f"Unknown depth_model: {config.depth_model}")               # :225
    c = L.GcsVisfeatConfig()
    L.check(L.load().gcs_visfeat_config_defaults(C.byref(c)), None, "gcs_visfeat_config_defaults")
    for f in fields(config):
        v = getattr(config, f.name)
        setattr(c, f.name, {"depth_sample_mode": _MODES, "depth_model": _MODELS}.get(f.name, {}).get(v, v))
    c.device = int(device)
    return c


def config_defaults() -> VisualFeatureConfig:
    """gcs_visfeat_config_defaults as a VisualFeatureConfig."""
    c = L.GcsVisfeatConfig()
    L.check(L.load().gcs_visfeat_config_defaults(C.byref(c)), None, "gcs_visfeat_config_defaults")
    names = {v: k for k, v in _MODES.items()}, {v: k for k, v in _MODELS.items()}
    kw = {f.name: getattr(c, f.name) for f in fields(VisualFeatureConfig)}
    kw["depth_sample_mode"], kw["depth_model"] = names[0][c.depth_sample_mode], names[1][c.depth_model]
    return VisualFeatureConfig(**kw)


def _keypoint_arrays(keypoints):
    """(u, v, response) as three arrays: from an (n, 3) array (or a list of n triples), or from a tuple / list
    of three 1-D arrays or tensors."""
    if isinstance(keypoints, (tuple, list)) and len(keypoints) == 3 and \
            all(hasattr(k, "shape") and len(k.shape) == 1 for k in keypoints):
        return tuple(keypoints)
    k = keypoints if hasattr(keypoints, "shape") else np.asarray(keypoints, np.float32).reshape(-1, 3)
    if k.ndim != 2 or k.shape[1] != 3:
        raise ValueError("keypoints: an (n, 3) array of u, v, response, or three arrays")
    return k[:, 0], k[:, 1], k[:, 2]


class _Features(dict):
    """Host feature arrays with .count and .diag."""


def _output_layout(rows: int, want_diag: bool):
    """Byte spans of gcs_visfeat_outputs' arrays in one allocation: 8-byte values first, then 4, then 1."""
    flds = L.VISFEAT_FEATURE_FIELDS + (L.VISFEAT_DIAG_FIELDS if want_diag else ())
    off, spans = 0, []
    for name, w, dt in sorted(flds, key=lambda f: -np.dtype(f[2]).itemsize):
        z = rows * max(w, 1) * np.dtype(dt).itemsize
        spans.append((name, off, z, dt, (rows, w) if w else (rows,)))
        off += z
    return spans, (off + 7) // 8 * 8


def _inputs_struct(depth_ptr, depth_format, depth_pitch, width, height, rgb_ptr, rgb_pitch, intrinsics, n, kp_ptrs):
    i = L.GcsVisfeatInputs()
    i.depth, i.depth_format, i.depth_pitch = depth_ptr, int(depth_format), int(depth_pitch)
    i.width, i.height = int(width), int(height)
    i.rgb, i.rgb_pitch = rgb_ptr, int(rgb_pitch)
    i.fx, i.fy, i.cx, i.cy = (float(getattr(intrinsics, k)) for k in ("fx", "fy", "cx", "cy"))
    i.n_keypoints = int(n)
    i.kp_u, i.kp_v, i.kp_response = kp_ptrs
    return i


class VisualFeatureExtractor:
    """A gcs_visfeat_ctx: the selection workspace for up to config.max_keypoints keypoints on one GPU."""

    def __init__(self, config: Optional[VisualFeatureConfig] = None, device: int = 0):
        self.config = config or VisualFeatureConfig()
        self.lib = L.load()
        c = config_struct(self.config, device)
        h = C.c_void_p()
        rc = self.lib.gcs_visfeat_ctx_create(C.byref(c), C.byref(h))
        if rc != 0:
            raise (ValueError if rc == -1 else RuntimeError)(f"gcs_visfeat_ctx_create failed ({rc})")
        self.h, self.device = h, int(device)

    def close(self):
        if getattr(self, "h", None):
            self.lib.gcs_visfeat_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc != 0:
            msg = self.lib.gcs_visfeat_last_error(self.h).decode(errors="replace")
            raise (ValueError if rc in (-1, -3) else RuntimeError)(f"{what} failed ({rc}): {msg}")

    def _image(self, x, kinds):
        """x (numpy or torch) as a device tensor of one of the dtypes `kinds` (the first when it has another),
        its rows contiguous; a torch tensor's row pitch is kept."""
        import torch
        dev = torch.device(f"cuda:{self.device}")
        if not torch.is_tensor(x):
            a = np.asarray(x)
            a = np.ascontiguousarray(a, a.dtype if a.dtype in kinds else kinds[0])
            if a.dtype == np.uint16:   # uploaded as its bits
                return torch.from_numpy(a.view(np.int16)).to(dev).view(torch.uint16)
            return torch.from_numpy(a).to(dev)
        x = x.to(dev)
        if x.dtype not in [getattr(torch, np.dtype(k).name) for k in kinds]:
            x = x.to(getattr(torch, np.dtype(kinds[0]).name))
        if x.shape[0] == 0 or not x[0].is_contiguous() or x.stride(0) < x[0].numel():
            x = x.contiguous()
        return x

    def extract(self, depth, rgb, keypoints, intrinsics: PinholeIntrinsics, want_diag: bool = False,
                trim: bool = True, keypoint_config: Optional[Union[KeypointConfig, PyramidConfig, GridConfig]] = None) -> _DeviceFeatures:
        """One frame's features as gcslam.camera's device feature dict, on the current torch stream and
        without waiting for it.  depth: (H, W) float32 or uint16 (metres = value * depth_scale), rgb:
        (H, W, 3) uint8 or None; torch device tensors, or numpy arrays (uploaded once).  keypoints: (n, 3)
        u, v, response or three arrays.  The dict's arrays hold .count = min(n, max_features) rows (trim
        False: all max_features, zeros beyond count); .diag (want_diag) the per-feature diagnostics.
        keypoints None: detected from rgb (gcslam.keypoints.detect_keypoints with keypoint_config, or with a
        PyramidConfig detect_keypoints_pyramid, with a GridConfig detect_keypoints_grid) on the same stream; that route waits once, for the detector's
        counts words."""
        import torch
        if keypoints is None and rgb is None:
            raise ValueError("keypoints=None needs rgb: the keypoints are detected from it")
        dev = torch.device(f"cuda:{self.device}")
        d = self._image(depth, (np.float32, np.uint16))
        if d.ndim != 2:
            raise ValueError("depth: an (H, W) image")
        H, W = int(d.shape[0]), int(d.shape[1])
        c = None
        if rgb is not None:
            c = self._image(rgb, (np.uint8,))
            if tuple(c.shape) != (H, W, 3):
                raise ValueError(f"rgb: shape {tuple(c.shape)}, expected {(H, W, 3)}")
        if keypoints is None:
            if isinstance(keypoint_config, GridConfig):
                keypoints = detect_keypoints_grid(c, keypoint_config, self.device)
            elif isinstance(keypoint_config, PyramidConfig):
                keypoints = detect_keypoints_pyramid(c, keypoint_config, self.device)
            else:
                keypoints = detect_keypoints(c, keypoint_config, self.device)
        kp = [torch.as_tensor(np.asarray(k, np.float32) if not torch.is_tensor(k) else k).to(dev, torch.float32)
              .contiguous() for k in _keypoint_arrays(keypoints)]
        n = int(kp[0].shape[0])
        if any(int(k.shape[0]) != n or k.ndim != 1 for k in kp):
            raise ValueError("keypoints: u, v and response differ in length")
        rows = int(self.config.max_features)
        spans, nbytes = _output_layout(rows, want_diag)
        buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        arrs = {name: buf[o:o + z].view(getattr(torch, dt)).view(sh) for name, o, z, dt, sh in spans}
        i = _inputs_struct(d.data_ptr(), 1 if d.dtype == torch.uint16 else 0, d.stride(0) * d.element_size(), W, H,
                           c.data_ptr() if c is not None else None, c.stride(0) if c is not None else 0, intrinsics,
                           n, [k.data_ptr() for k in kp])
        o = L.GcsVisfeatOutputs()
        for name, x in arrs.items():
            setattr(o, name, x.data_ptr())
        self._chk(self.lib.gcs_visfeat_ctx_set_stream(self.h, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
                  "gcs_visfeat_ctx_set_stream")
        self._chk(self.lib.gcs_visual_features(self.h, C.byref(i), C.byref(o)), "gcs_visual_features")
        m = int(o.count) if trim else rows
        out = _DeviceFeatures((name, arrs[name][:m]) for name, _, _ in L.VISFEAT_FEATURE_FIELDS)
        out.count = int(o.count)
        out.diag = {name: arrs[name][:m] for name, _, _ in L.VISFEAT_DIAG_FIELDS} if want_diag else None
        return out


_extractors = {}


def _extractor_for(config, device) -> VisualFeatureExtractor:
    key = (config, int(device))
    e = _extractors.get(key)
    if e is None or e.h is None:
        e = _extractors[key] = VisualFeatureExtractor(config, device)
    return e


def extract_visual_features(depth, rgb, keypoints, intrinsics: PinholeIntrinsics,
                            config: Optional[VisualFeatureConfig] = None, device: int = 0, want_diag: bool = False,
                            trim: bool = True, keypoint_config: Optional[Union[KeypointConfig, PyramidConfig, GridConfig]] = None) -> _DeviceFeatures:
    """VisualFeatureExtractor.extract on a cached extractor of (config, device)."""
    return _extractor_for(config or VisualFeatureConfig(), device).extract(depth, rgb, keypoints, intrinsics,
                                                                           want_diag=want_diag, trim=trim,
                                                                           keypoint_config=keypoint_config)


def visual_features_host(depth, rgb, keypoints, intrinsics: PinholeIntrinsics,
                         config: Optional[VisualFeatureConfig] = None, want_diag: bool = False,
                         trim: bool = True) -> _Features:
    """The same rows through gcs_visual_features_host: the kernel's per-keypoint math built for the host,
    numpy arrays in and out, no device."""
    config = config or VisualFeatureConfig()
    c = config_struct(config, 0)
    d = np.asarray(depth)
    d = np.ascontiguousarray(d, d.dtype if d.dtype in (np.float32, np.uint16) else np.float32)
    if d.ndim != 2:
        raise ValueError("depth: an (H, W) image")
    H, W = d.shape
    col = None
    if rgb is not None:
        col = np.ascontiguousarray(rgb, np.uint8)
        if col.shape != (H, W, 3):
            raise ValueError(f"rgb: shape {col.shape}, expected {(H, W, 3)}")
    kp = [np.ascontiguousarray(k, np.float32) for k in _keypoint_arrays(keypoints)]
    n = kp[0].shape[0]
    if any(k.shape != (n,) for k in kp):
        raise ValueError("keypoints: u, v and response differ in length")
    rows = int(config.max_features)
    flds = L.VISFEAT_FEATURE_FIELDS + (L.VISFEAT_DIAG_FIELDS if want_diag else ())
    arrs = {name: np.empty((rows, w) if w else (rows,), dt) for name, w, dt in flds}
    i = _inputs_struct(d.ctypes.data, 1 if d.dtype == np.uint16 else 0, d.strides[0], W, H,
                       col.ctypes.data if col is not None else None, col.strides[0] if col is not None else 0,
                       intrinsics, n, [k.ctypes.data for k in kp])
    o = L.GcsVisfeatOutputs()
    for name, x in arrs.items():
        setattr(o, name, x.ctypes.data)
    rc = L.load().gcs_visual_features_host(C.byref(c), C.byref(i), C.byref(o))
    if rc != 0:
        raise ValueError(f"gcs_visual_features_host failed ({rc})")
    m = int(o.count) if trim else rows
    out = _Features((name, arrs[name][:m]) for name, _, _ in L.VISFEAT_FEATURE_FIELDS)
    out.count = int(o.count)
    out.diag = {name: arrs[name][:m] for name, _, _ in L.VISFEAT_DIAG_FIELDS} if want_diag else None
    return out


def camera_frame_from_rgbd(depth, rgb, keypoints, intrinsics: PinholeIntrinsics, R_base_camera, t_base_camera,
                           timestamp_sec: float, config: Optional[VisualFeatureConfig] = None,
                           fusion_config: Optional[DepthFusionConfig] = None, device: int = 0,
                           want_diag: bool = False, max_candidates: int = 1024,
                           keypoint_config: Optional[Union[KeypointConfig, PyramidConfig, GridConfig]] = None) -> CameraFrame:
    """on_rgbd after detectAndCompute, the VisualFeatureBatch and _feature_batch_to_list in one step: the
    frame's features extracted on the GPU and held there in a CameraFrame for
    process_scan_single_hypothesis(camera_batch=..., camera_batch_policy="use").  keypoints None: detectAndCompute's
    detector front as well, from rgb (gcslam.keypoints), so a node without a detector of its own passes the
    two images and nothing else."""
    feats = extract_visual_features(depth, rgb, keypoints, intrinsics, config=config, device=device,
                                    keypoint_config=keypoint_config)
    return CameraFrame(feats, intrinsics, R_base_camera, t_base_camera, timestamp_sec,
                       config=fusion_config or DepthFusionConfig(), want_diag=want_diag, max_candidates=max_candidates)
