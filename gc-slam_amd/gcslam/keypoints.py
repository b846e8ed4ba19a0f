"""Keypoints from an 8-bit image on the MI355X, through gcs_detect_keypoints (libgcslam_hip.so): the detector
front of the FAST / ORB recipe at pyramid level 0 -- grey conversion, the FAST-9/16 segment test and score,
strict 3 x 3 suppression, the border, the Harris response over a 7 x 7 block and the max_keypoints best by
(response descending, raster index ascending), written in raster order.  This detector is the project's own.
It follows the published FAST / ORB recipe, but it claims no parity with cv::ORB: there is no pyramid, there
is no orientation, and there are no descriptors.  The definition is in include/gcslam_hip.h; the result is
the (u, v, response) triple gcslam.visual takes as `keypoints`, device to device."""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, fields, replace
from typing import Optional

import numpy as np

from . import _lib as L


@dataclass(frozen=True)
class KeypointConfig:
    """gcs_keypoint_config: ORB's fastThreshold and edgeThreshold, the cap, the workspace's capacity, Harris' k."""
    fast_threshold: int = 20
    edge_threshold: int = 31
    max_keypoints: int = 4096
    max_width: int = 1920
    max_height: int = 1080
    harris_k: float = 0.04


def config_struct(config: Optional[KeypointConfig] = None, device: int = 0) -> "L.GcsKeypointConfig":
    """gcs_keypoint_config of a KeypointConfig."""
    config = config or KeypointConfig()
    c = L.GcsKeypointConfig()
    L.check(L.load().gcs_keypoint_config_defaults(C.byref(c)), None, "gcs_keypoint_config_defaults")
    for f in fields(config):
        setattr(c, f.name, getattr(config, f.name))
    c.device = int(device)
    return c


def config_defaults() -> KeypointConfig:
    """gcs_keypoint_config_defaults as a KeypointConfig."""
    c = L.GcsKeypointConfig()
    L.check(L.load().gcs_keypoint_config_defaults(C.byref(c)), None, "gcs_keypoint_config_defaults")
    return KeypointConfig(**{f.name: getattr(c, f.name) for f in fields(KeypointConfig)})


class Keypoints(tuple):
    """(u, v, response), each of n_keypoints float32 values in raster order, with .counts = (n_keypoints,
    n_survivors, n_corners, 0): a valid `keypoints` argument of gcslam.visual."""
    counts = (0, 0, 0, 0)


def _inputs_struct(ptr, channels, pitch, width, height):
    i = L.GcsKeypointInputs()
    i.image, i.channels, i.pitch, i.width, i.height = ptr, int(channels), int(pitch), int(width), int(height)
    return i


def _shape(shape):
    if len(shape) == 2:
        return int(shape[0]), int(shape[1]), 1
    if len(shape) == 3 and shape[2] == 3:
        return int(shape[0]), int(shape[1]), 3
    raise ValueError(f"image: shape {tuple(shape)}, expected (H, W) or (H, W, 3)")


class KeypointDetector:
    """A gcs_keypoint_ctx: the per-pixel workspace for images up to config.max_width x config.max_height on
    one GPU."""

    def __init__(self, config: Optional[KeypointConfig] = None, device: int = 0):
        self.config = config or KeypointConfig()
        self.lib = L.load()
        c = config_struct(self.config, device)
        h = C.c_void_p()
        rc = self.lib.gcs_keypoint_ctx_create(C.byref(c), C.byref(h))
        if rc != 0:
            raise (ValueError if rc == -1 else RuntimeError)(f"gcs_keypoint_ctx_create failed ({rc})")
        self.h, self.device = h, int(device)
        self._pinned = None

    def close(self):
        if getattr(self, "h", None):
            self.lib.gcs_keypoint_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc != 0:
            msg = self.lib.gcs_keypoint_last_error(self.h).decode(errors="replace")
            raise (ValueError if rc in (-1, -3) else RuntimeError)(f"{what} failed ({rc}): {msg}")

    def _image(self, x):
        """x (numpy or torch) as a uint8 device tensor whose pixels are contiguous within a row; a torch view's
        row pitch is kept."""
        import torch
        dev = torch.device(f"cuda:{self.device}")
        if not torch.is_tensor(x):
            x = torch.from_numpy(np.ascontiguousarray(x, np.uint8))
        if x.dtype != torch.uint8:
            raise ValueError(f"image: dtype {x.dtype}, expected uint8")
        x = x.to(dev)
        H, W, ch = _shape(x.shape)
        packed = x.stride(1) == ch and (ch == 1 or x.stride(2) == 1)
        if H == 0 or W == 0 or not packed or x.stride(0) < W * ch:
            x = x.contiguous()
        return x, H, W, ch

    def queue(self, image):
        """gcs_detect_keypoints on the current torch stream, without waiting: (u, v, response) of all
        max_keypoints rows (NaN beyond the count) and the device counts word."""
        import torch
        dev = torch.device(f"cuda:{self.device}")
        x, H, W, ch = self._image(image)
        K = int(self.config.max_keypoints)
        buf = torch.empty(3 * K + 4, dtype=torch.float32, device=dev)
        counts = buf[3 * K:].view(torch.int32)
        i = _inputs_struct(x.data_ptr(), ch, x.stride(0), W, H)
        o = L.GcsKeypointOutputs()
        o.kp_u, o.kp_v, o.kp_response = (buf[j * K:].data_ptr() for j in range(3))
        o.counts = counts.data_ptr()
        self._chk(self.lib.gcs_keypoint_ctx_set_stream(self.h, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
                  "gcs_keypoint_ctx_set_stream")
        self._chk(self.lib.gcs_detect_keypoints(self.h, C.byref(i), C.byref(o)), "gcs_detect_keypoints")
        return tuple(buf[j * K:(j + 1) * K] for j in range(3)), counts

    def detect(self, image) -> Keypoints:
        """One image's keypoints: (u, v, response) device tensors trimmed to the count, with .counts.  image:
        (H, W) gray8 or (H, W, 3) rgb8, uint8; a torch device tensor (a view's row pitch is kept) or a numpy
        array (uploaded once).  The kernels are queued on the current torch stream.  The call waits for the
        16-byte counts word -- a read-back into pinned memory -- and for nothing else: that is its one
        synchronisation, needed because the result's length is decided on the device."""
        import torch
        rows, counts = self.queue(image)
        if self._pinned is None:
            self._pinned = torch.empty(4, dtype=torch.int32).pin_memory()
        self._pinned.copy_(counts, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(torch.device(f"cuda:{self.device}")))
        ev.synchronize()
        c = tuple(int(v) for v in self._pinned.tolist())
        out = Keypoints(r[:c[0]] for r in rows)
        out.counts = c
        return out


_detectors = {}


def _detector_for(config: KeypointConfig, device: int, height: int, width: int) -> KeypointDetector:
    """The cached detector of (config, device); its capacity grows to the largest image seen."""
    key = (replace(config, max_width=0, max_height=0), int(device))
    d = _detectors.get(key)
    if d is None or d.h is None or d.config.max_width < width or d.config.max_height < height:
        have = d.config if d is not None else config
        if d is not None:
            d.close()
        d = _detectors[key] = KeypointDetector(replace(config, max_width=max(have.max_width, config.max_width, width),
                                                       max_height=max(have.max_height, config.max_height, height)), device)
    return d


def detect_keypoints(image, config: Optional[KeypointConfig] = None, device: int = 0) -> Keypoints:
    """KeypointDetector.detect on a cached detector of (config, device)."""
    H, W, _ = _shape(image.shape)
    return _detector_for(config or KeypointConfig(), device, H, W).detect(image)


def detect_keypoints_host(image, config: Optional[KeypointConfig] = None, pitch: Optional[int] = None,
                          shape=None, trim: bool = True) -> Keypoints:
    """The same steps through gcs_detect_keypoints_host: numpy in and out, no device.  image: (H, W) or
    (H, W, 3) uint8; or, with pitch and shape = (H, W, channels), a flat uint8 buffer whose rows are pitch
    bytes apart.  trim False: all max_keypoints rows, NaN beyond the count."""
    config = config or KeypointConfig()
    a = np.ascontiguousarray(image, np.uint8)
    if pitch is None:
        H, W, ch = _shape(a.shape)
        pitch = W * ch
    else:
        H, W, ch = (int(v) for v in shape)
        if a.ndim != 1 or H < 1 or a.size < (H - 1) * pitch + W * ch:
            raise ValueError("image: a flat buffer of at least (H - 1) * pitch + W * channels bytes")
    c = config_struct(replace(config, max_width=max(config.max_width, W), max_height=max(config.max_height, H)), 0)
    K = int(config.max_keypoints)
    rows = [np.empty(max(K, 0), np.float32) for _ in range(3)]
    counts = np.zeros(4, np.int32)
    i = _inputs_struct(a.ctypes.data, ch, pitch, W, H)
    o = L.GcsKeypointOutputs()
    o.kp_u, o.kp_v, o.kp_response = (r.ctypes.data for r in rows)
    o.counts = counts.ctypes.data
    rc = L.load().gcs_detect_keypoints_host(C.byref(c), C.byref(i), C.byref(o))
    if rc != 0:
        raise ValueError(f"gcs_detect_keypoints_host failed ({rc})")
    out = Keypoints(r[:int(counts[0])] if trim else r for r in rows)
    out.counts = tuple(int(v) for v in counts)
    return out
