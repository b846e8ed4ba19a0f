"""Keypoints from an 8-bit image on the MI355X, through gcs_detect_keypoints (libgcslam_hip.so): the detector
front of the FAST / ORB recipe at pyramid level 0 -- grey conversion, the FAST-9/16 segment test and score,
strict 3 x 3 suppression, the border, the Harris response over a 7 x 7 block and the max_keypoints best by
(response descending, raster index ascending), written in raster order.  This detector is the project's own.
It follows the published FAST / ORB recipe, but it claims no parity with cv::ORB: there is no pyramid here
(PyramidDetector, below), and orientation and descriptors are gcslam.descriptors' own operators.  The definition
is in include/gcslam_hip.h; the result is the (u, v, response) triple gcslam.visual takes as `keypoints`, device
to device.

PyramidDetector (gcs_detect_keypoints_pyramid) runs the same detector over a scale pyramid -- n_levels exact
pixel-area resamples of the grey image at the rational scale scale_num / scale_den, a fixed quota of
max_keypoints per level -- and reports every keypoint in level-0 pixel coordinates with its level.

GridDetector (gcs_detect_keypoints_grid) is the pyramid detector with each level's selection replaced by a fair
share among the cells of a grid over the level, so that the kept keypoints spread over the image, and with a
level's unused quota handed on to the levels that have survivors to spare (finest first)."""

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


# ---- the scale pyramid

@dataclass(frozen=True)
class PyramidConfig:
    """gcs_keypoint_pyramid_config: KeypointConfig's six fields, ORB's nlevels and its scaleFactor as the rational
    scale_num / scale_den."""
    fast_threshold: int = 20
    edge_threshold: int = 31
    max_keypoints: int = 4096
    max_width: int = 1920
    max_height: int = 1080
    harris_k: float = 0.04
    n_levels: int = 8
    scale_num: int = 6
    scale_den: int = 5


MAX_LEVELS = L.KEYPOINT_MAX_LEVELS
_WORDS = 4 + 4 * MAX_LEVELS   # counts, then level_counts


def pyramid_config_struct(config: Optional[PyramidConfig] = None, device: int = 0) -> "L.GcsKeypointPyramidConfig":
    """gcs_keypoint_pyramid_config of a PyramidConfig."""
    config = config or PyramidConfig()
    c = L.GcsKeypointPyramidConfig()
    L.check(L.load().gcs_keypoint_pyramid_config_defaults(C.byref(c)), None, "gcs_keypoint_pyramid_config_defaults")
    for f in fields(config):
        setattr(c, f.name, getattr(config, f.name))
    c.device = int(device)
    return c


def pyramid_config_defaults() -> PyramidConfig:
    """gcs_keypoint_pyramid_config_defaults as a PyramidConfig."""
    c = L.GcsKeypointPyramidConfig()
    L.check(L.load().gcs_keypoint_pyramid_config_defaults(C.byref(c)), None, "gcs_keypoint_pyramid_config_defaults")
    return PyramidConfig(**{f.name: getattr(c, f.name) for f in fields(PyramidConfig)})


def pyramid_layout(config: Optional[PyramidConfig], width: int, height: int):
    """gcs_keypoint_pyramid_layout: an (8, 3) int32 array of W_l, H_l, quota_l."""
    out = np.zeros((MAX_LEVELS, 3), np.int32)
    c = pyramid_config_struct(config, 0)
    if L.load().gcs_keypoint_pyramid_layout(C.byref(c), int(width), int(height), out.ctypes.data) != 0:
        raise ValueError("gcs_keypoint_pyramid_layout: a config or an image size outside its range")
    return out


class PyramidKeypoints(Keypoints):
    """Keypoints in (level, raster index) order, u and v in level-0 pixels, with .counts = (n_keypoints,
    n_survivors, n_corners, n_levels), .level (int32, one per row) and .level_counts (per level: n_keypoints,
    n_survivors, n_corners, quota)."""
    level = None
    level_counts = ((0, 0, 0, 0),) * MAX_LEVELS


def _pyramid_result(rows, level, words, n=None, cols=4):
    out = PyramidKeypoints(r if n is None else r[:n] for r in rows)
    out.level = level if n is None else level[:n]
    out.counts = tuple(int(v) for v in words[:4])
    out.level_counts = tuple(tuple(int(v) for v in words[4 + cols * l:4 + cols * (l + 1)]) for l in range(MAX_LEVELS))
    return out


class PyramidDetector(KeypointDetector):
    """A gcs_keypoint_pyramid_ctx: the packed per-pixel workspace of every level for images up to
    config.max_width x config.max_height on one GPU."""

    def __init__(self, config: Optional[PyramidConfig] = None, device: int = 0):
        self.config = config or PyramidConfig()
        self.lib = L.load()
        c = pyramid_config_struct(self.config, device)
        h = C.c_void_p()
        rc = self.lib.gcs_keypoint_pyramid_ctx_create(C.byref(c), C.byref(h))
        if rc != 0:
            raise (ValueError if rc == -1 else RuntimeError)(f"gcs_keypoint_pyramid_ctx_create failed ({rc})")
        self.h, self.device = h, int(device)
        self._pinned = None

    def close(self):
        if getattr(self, "h", None):
            self.lib.gcs_keypoint_pyramid_ctx_destroy(self.h)
            self.h = None

    def _chk(self, rc, what):
        if rc != 0:
            msg = self.lib.gcs_keypoint_pyramid_last_error(self.h).decode(errors="replace")
            raise (ValueError if rc in (-1, -3) else RuntimeError)(f"{what} failed ({rc}): {msg}")

    def queue(self, image):
        """gcs_detect_keypoints_pyramid on the current torch stream, without waiting: ((u, v, response) of all
        max_keypoints rows, NaN beyond the count; the rows' levels, -1 beyond it; the 36 device words of counts
        and level_counts)."""
        import torch
        dev = torch.device(f"cuda:{self.device}")
        x, H, W, ch = self._image(image)
        K = int(self.config.max_keypoints)
        buf = torch.empty(4 * K + _WORDS, dtype=torch.float32, device=dev)
        level, words = buf[3 * K:4 * K].view(torch.int32), buf[4 * K:].view(torch.int32)
        i = _inputs_struct(x.data_ptr(), ch, x.stride(0), W, H)
        o = L.GcsKeypointPyramidOutputs()
        o.kp_u, o.kp_v, o.kp_response, o.kp_level = (buf[j * K:].data_ptr() for j in range(4))
        o.counts, o.level_counts = words.data_ptr(), words[4:].data_ptr()
        self._chk(self.lib.gcs_keypoint_pyramid_ctx_set_stream(
            self.h, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "gcs_keypoint_pyramid_ctx_set_stream")
        self._chk(self.lib.gcs_detect_keypoints_pyramid(self.h, C.byref(i), C.byref(o)), "gcs_detect_keypoints_pyramid")
        return tuple(buf[j * K:(j + 1) * K] for j in range(3)), level, words

    def detect(self, image) -> PyramidKeypoints:
        """One image's keypoints over the pyramid: (u, v, response) device tensors trimmed to the count, with
        .level (device int32), .counts and .level_counts.  image as KeypointDetector.detect's.  The call waits
        once, for the 144 bytes of counts and level_counts read back into pinned memory together."""
        import torch
        rows, level, words = self.queue(image)
        if self._pinned is None:
            self._pinned = torch.empty(_WORDS, dtype=torch.int32).pin_memory()
        self._pinned.copy_(words, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(torch.device(f"cuda:{self.device}")))
        ev.synchronize()
        w = self._pinned.tolist()
        return _pyramid_result(rows, level, w, w[0])


_pyramid_detectors = {}


def _pyramid_detector_for(config: PyramidConfig, device: int, height: int, width: int) -> PyramidDetector:
    """The cached pyramid detector of (config, device); its capacity grows to the largest image seen."""
    key = (replace(config, max_width=0, max_height=0), int(device))
    d = _pyramid_detectors.get(key)
    if d is None or d.h is None or d.config.max_width < width or d.config.max_height < height:
        have = d.config if d is not None else config
        if d is not None:
            d.close()
        d = _pyramid_detectors[key] = PyramidDetector(
            replace(config, max_width=max(have.max_width, config.max_width, width),
                    max_height=max(have.max_height, config.max_height, height)), device)
    return d


def detect_keypoints_pyramid(image, config: Optional[PyramidConfig] = None, device: int = 0) -> PyramidKeypoints:
    """PyramidDetector.detect on a cached detector of (config, device)."""
    H, W, _ = _shape(image.shape)
    return _pyramid_detector_for(config or PyramidConfig(), device, H, W).detect(image)


def detect_keypoints_pyramid_host(image, config: Optional[PyramidConfig] = None, pitch: Optional[int] = None,
                                  shape=None, trim: bool = True) -> PyramidKeypoints:
    """The same steps through gcs_detect_keypoints_pyramid_host: numpy in and out, no device.  Arguments as
    detect_keypoints_host's."""
    config = config or PyramidConfig()
    a = np.ascontiguousarray(image, np.uint8)
    if pitch is None:
        H, W, ch = _shape(a.shape)
        pitch = W * ch
    else:
        H, W, ch = (int(v) for v in shape)
        if a.ndim != 1 or H < 1 or a.size < (H - 1) * pitch + W * ch:
            raise ValueError("image: a flat buffer of at least (H - 1) * pitch + W * channels bytes")
    c = pyramid_config_struct(replace(config, max_width=max(config.max_width, W), max_height=max(config.max_height, H)), 0)
    K = int(config.max_keypoints)
    rows = [np.empty(max(K, 0), np.float32) for _ in range(3)]
    level = np.empty(max(K, 0), np.int32)
    words = np.zeros(_WORDS, np.int32)
    i = _inputs_struct(a.ctypes.data, ch, pitch, W, H)
    o = L.GcsKeypointPyramidOutputs()
    o.kp_u, o.kp_v, o.kp_response = (r.ctypes.data for r in rows)
    o.kp_level, o.counts, o.level_counts = level.ctypes.data, words.ctypes.data, words[4:].ctypes.data
    rc = L.load().gcs_detect_keypoints_pyramid_host(C.byref(c), C.byref(i), C.byref(o))
    if rc != 0:
        raise ValueError(f"gcs_detect_keypoints_pyramid_host failed ({rc})")
    return _pyramid_result(rows, level, words.tolist(), int(words[0]) if trim else None)


# ---- the grid of cells

@dataclass(frozen=True)
class GridConfig:
    """gcs_keypoint_grid_config: PyramidConfig's fields, the side of a cell in level pixels and whether a level's
    unused quota is handed on."""
    fast_threshold: int = 20
    edge_threshold: int = 31
    max_keypoints: int = 4096
    max_width: int = 1920
    max_height: int = 1080
    harris_k: float = 0.04
    n_levels: int = 8
    scale_num: int = 6
    scale_den: int = 5
    cell_size: int = 32
    redistribute: bool = True


GRID_COLUMNS = 6   # level_counts: n_keypoints, n_survivors, n_corners, quota, budget, cap
_GRID_WORDS = 4 + GRID_COLUMNS * MAX_LEVELS


def grid_config_struct(config: Optional[GridConfig] = None, device: int = 0) -> "L.GcsKeypointGridConfig":
    """gcs_keypoint_grid_config of a GridConfig."""
    config = config or GridConfig()
    c = L.GcsKeypointGridConfig()
    L.check(L.load().gcs_keypoint_grid_config_defaults(C.byref(c)), None, "gcs_keypoint_grid_config_defaults")
    for f in fields(config):
        setattr(c, f.name, getattr(config, f.name))
    c.device = int(device)
    return c


def grid_config_defaults() -> GridConfig:
    """gcs_keypoint_grid_config_defaults as a GridConfig."""
    c = L.GcsKeypointGridConfig()
    L.check(L.load().gcs_keypoint_grid_config_defaults(C.byref(c)), None, "gcs_keypoint_grid_config_defaults")
    got = {f.name: getattr(c, f.name) for f in fields(GridConfig)}
    return GridConfig(**dict(got, redistribute=bool(got["redistribute"])))


def grid_layout(config: Optional[GridConfig], width: int, height: int):
    """gcs_keypoint_grid_layout: an (8, 5) int32 array of W_l, H_l, quota_l, n_cx, n_cy."""
    out = np.zeros((MAX_LEVELS, 5), np.int32)
    c = grid_config_struct(config, 0)
    if L.load().gcs_keypoint_grid_layout(C.byref(c), int(width), int(height), out.ctypes.data) != 0:
        raise ValueError("gcs_keypoint_grid_layout: a config or an image size outside its range")
    return out


class GridDetector(PyramidDetector):
    """A gcs_keypoint_grid_ctx: the pyramid's packed workspace and a second key image for images up to
    config.max_width x config.max_height on one GPU.  queue, detect and close as PyramidDetector's; the result's
    level_counts has six columns (n_keypoints, n_survivors, n_corners, quota, budget, cap)."""

    def __init__(self, config: Optional[GridConfig] = None, device: int = 0):
        self.config = config or GridConfig()
        self.lib = L.load()
        c = grid_config_struct(self.config, device)
        h = C.c_void_p()
        rc = self.lib.gcs_keypoint_grid_ctx_create(C.byref(c), C.byref(h))
        if rc != 0:
            raise (ValueError if rc == -1 else RuntimeError)(f"gcs_keypoint_grid_ctx_create failed ({rc})")
        self.h, self.device = h, int(device)
        self._pinned = None

    def close(self):
        if getattr(self, "h", None):
            self.lib.gcs_keypoint_grid_ctx_destroy(self.h)
            self.h = None

    def _chk(self, rc, what):
        if rc != 0:
            msg = self.lib.gcs_keypoint_grid_last_error(self.h).decode(errors="replace")
            raise (ValueError if rc in (-1, -3) else RuntimeError)(f"{what} failed ({rc}): {msg}")

    def queue(self, image):
        """gcs_detect_keypoints_grid on the current torch stream, without waiting: ((u, v, response) of all
        max_keypoints rows, NaN beyond the count; the rows' levels, -1 beyond it; the 52 device words of counts
        and level_counts)."""
        import torch
        dev = torch.device(f"cuda:{self.device}")
        x, H, W, ch = self._image(image)
        K = int(self.config.max_keypoints)
        buf = torch.empty(4 * K + _GRID_WORDS, dtype=torch.float32, device=dev)
        level, words = buf[3 * K:4 * K].view(torch.int32), buf[4 * K:].view(torch.int32)
        i = _inputs_struct(x.data_ptr(), ch, x.stride(0), W, H)
        o = L.GcsKeypointGridOutputs()
        o.kp_u, o.kp_v, o.kp_response, o.kp_level = (buf[j * K:].data_ptr() for j in range(4))
        o.counts, o.level_counts = words.data_ptr(), words[4:].data_ptr()
        self._chk(self.lib.gcs_keypoint_grid_ctx_set_stream(
            self.h, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "gcs_keypoint_grid_ctx_set_stream")
        self._chk(self.lib.gcs_detect_keypoints_grid(self.h, C.byref(i), C.byref(o)), "gcs_detect_keypoints_grid")
        return tuple(buf[j * K:(j + 1) * K] for j in range(3)), level, words

    def detect(self, image) -> PyramidKeypoints:
        """One image's keypoints, spread over the grid: as PyramidDetector.detect, with the six-column
        level_counts.  The call waits once, for the 208 bytes of counts and level_counts."""
        import torch
        rows, level, words = self.queue(image)
        if self._pinned is None:
            self._pinned = torch.empty(_GRID_WORDS, dtype=torch.int32).pin_memory()
        self._pinned.copy_(words, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(torch.device(f"cuda:{self.device}")))
        ev.synchronize()
        w = self._pinned.tolist()
        return _pyramid_result(rows, level, w, w[0], GRID_COLUMNS)


_grid_detectors = {}


def _grid_detector_for(config: GridConfig, device: int, height: int, width: int) -> GridDetector:
    """The cached grid detector of (config, device); its capacity grows to the largest image seen."""
    key = (replace(config, max_width=0, max_height=0), int(device))
    d = _grid_detectors.get(key)
    if d is None or d.h is None or d.config.max_width < width or d.config.max_height < height:
        have = d.config if d is not None else config
        if d is not None:
            d.close()
        d = _grid_detectors[key] = GridDetector(
            replace(config, max_width=max(have.max_width, config.max_width, width),
                    max_height=max(have.max_height, config.max_height, height)), device)
    return d


def detect_keypoints_grid(image, config: Optional[GridConfig] = None, device: int = 0) -> PyramidKeypoints:
    """GridDetector.detect on a cached detector of (config, device)."""
    H, W, _ = _shape(image.shape)
    return _grid_detector_for(config or GridConfig(), device, H, W).detect(image)


def detect_keypoints_grid_host(image, config: Optional[GridConfig] = None, pitch: Optional[int] = None,
                               shape=None, trim: bool = True) -> PyramidKeypoints:
    """The same steps through gcs_detect_keypoints_grid_host: numpy in and out, no device.  Arguments as
    detect_keypoints_host's."""
    config = config or GridConfig()
    a = np.ascontiguousarray(image, np.uint8)
    if pitch is None:
        H, W, ch = _shape(a.shape)
        pitch = W * ch
    else:
        H, W, ch = (int(v) for v in shape)
        if a.ndim != 1 or H < 1 or a.size < (H - 1) * pitch + W * ch:
            raise ValueError("image: a flat buffer of at least (H - 1) * pitch + W * channels bytes")
    c = grid_config_struct(replace(config, max_width=max(config.max_width, W), max_height=max(config.max_height, H)), 0)
    K = int(config.max_keypoints)
    rows = [np.empty(max(K, 0), np.float32) for _ in range(3)]
    level = np.empty(max(K, 0), np.int32)
    words = np.zeros(_GRID_WORDS, np.int32)
    i = _inputs_struct(a.ctypes.data, ch, pitch, W, H)
    o = L.GcsKeypointGridOutputs()
    o.kp_u, o.kp_v, o.kp_response = (r.ctypes.data for r in rows)
    o.kp_level, o.counts, o.level_counts = level.ctypes.data, words.ctypes.data, words[4:].ctypes.data
    rc = L.load().gcs_detect_keypoints_grid_host(C.byref(c), C.byref(i), C.byref(o))
    if rc != 0:
        raise ValueError(f"gcs_detect_keypoints_grid_host failed ({rc})")
    return _pyramid_result(rows, level, words.tolist(), int(words[0]) if trim else None, GRID_COLUMNS)
