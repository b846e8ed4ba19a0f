"""Keypoint descriptors and their matcher on the MI355X, through gcs_describe_keypoints and gcs_match_descriptors
(libgcslam_hip.so): behind a detector of gcslam.keypoints, the intensity-centroid orientation of every keypoint on
its pyramid level, a 256-bit steered BRIEF descriptor, and brute-force Hamming matching of two descriptor sets
(nearest and second-nearest neighbour of every row).  The operators are the project's own (the definition: D1-D7
in include/gcslam_hip.h).  The test pattern is a fixed pseudo-random one (tools/gen_brief_pattern.py), not ORB's
learned rBRIEF pattern, and no parity with cv::ORB is claimed.  The angle bin, the 256 bits and every match output
are integer arithmetic: device, host twin and tests/keypoints_desc_ref.py agree as bytes.

gcs_match_descriptors_gated and gcs_match_pairs (D8, D9) match inside a search window and build the pairs on the
device: DescriptorMatcher.queue_gated and queue_pairs wait for nothing, match_pairs makes one wait for the 4-byte
count, and nearest_gated_host, pairs_host and match_pairs_host are the host twins; tests/keypoints_gate_ref.py is
their restatement.  match_descriptors is the earlier route, left as it was.

The describer's n_levels, scale_num and scale_den must be those of the detector whose keypoints it is given: they
decide the level images.  A single-level detector's result (no .level) is described on level 0."""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, fields, replace
from typing import Optional

import numpy as np

from . import _lib as L
from . import keypoints as KP

DESC_BYTES = L.DESC_BYTES
MATCH_NONE = L.MATCH_NONE


@dataclass(frozen=True)
class DescriptorConfig:
    """gcs_keypoint_desc_config: the pyramid's geometry, the workspace's capacity and the most keypoints of a call."""
    n_levels: int = 8
    scale_num: int = 6
    scale_den: int = 5
    max_width: int = 1920
    max_height: int = 1080
    max_keypoints: int = 4096


def config_struct(config: Optional[DescriptorConfig] = None, device: int = 0) -> "L.GcsKeypointDescConfig":
    """gcs_keypoint_desc_config of a DescriptorConfig."""
    config = config or DescriptorConfig()
    c = L.GcsKeypointDescConfig()
    L.check(L.load().gcs_keypoint_desc_config_defaults(C.byref(c)), None, "gcs_keypoint_desc_config_defaults")
    for f in fields(config):
        setattr(c, f.name, getattr(config, f.name))
    c.device = int(device)
    return c


def config_defaults() -> DescriptorConfig:
    """gcs_keypoint_desc_config_defaults as a DescriptorConfig."""
    c = L.GcsKeypointDescConfig()
    L.check(L.load().gcs_keypoint_desc_config_defaults(C.byref(c)), None, "gcs_keypoint_desc_config_defaults")
    return DescriptorConfig(**{f.name: getattr(c, f.name) for f in fields(DescriptorConfig)})


def config_like(detector_config, **over) -> DescriptorConfig:
    """The DescriptorConfig that goes with a KeypointConfig, PyramidConfig or GridConfig: its levels and capacity."""
    d = DescriptorConfig()
    names = [f.name for f in fields(DescriptorConfig)]
    got = {k: getattr(detector_config, k) for k in names if hasattr(detector_config, k)}
    if not hasattr(detector_config, "n_levels"):
        got["n_levels"] = 1
    return replace(d, **dict(got, **over))


def brief_pattern() -> np.ndarray:
    """gcs_brief_pattern: the (256, 4) int8 rows ax, ay, bx, by of D5."""
    out = np.zeros((256, 4), np.int8)
    L.check(L.load().gcs_brief_pattern(out.ctypes.data), None, "gcs_brief_pattern")
    return out


class Descriptors:
    """One call's result: .desc (n, 32) uint8, .angle (n,) float32 radians, .angle_bin (n,) int32 (-1: an invalid
    row, whose descriptor is zero and whose angle is NaN).  Device tensors from the device routes, numpy arrays
    from the host twin."""

    def __init__(self, desc, angle, angle_bin):
        self.desc, self.angle, self.angle_bin = desc, angle, angle_bin

    def __len__(self):
        return int(self.desc.shape[0])


def _keypoint_arrays(keypoints):
    """(u, v, level or None) of a Keypoints / PyramidKeypoints result or of a (u, v[, response[, level]]) tuple."""
    level = getattr(keypoints, "level", None)
    rows = tuple(keypoints)
    if len(rows) < 2:
        raise ValueError("keypoints: (u, v, ...) expected")
    if level is None and len(rows) >= 4:
        level = rows[3]
    return rows[0], rows[1], level


class KeypointDescriber:
    """A gcs_keypoint_desc_ctx: the packed grey images of every level for images up to config.max_width x
    config.max_height on one GPU."""

    _image = KP.KeypointDetector._image

    def __init__(self, config: Optional[DescriptorConfig] = None, device: int = 0):
        self.config = config or DescriptorConfig()
        self.lib = L.load()
        c = config_struct(self.config, device)
        h = C.c_void_p()
        rc = self.lib.gcs_keypoint_desc_ctx_create(C.byref(c), C.byref(h))
        if rc != 0:
            raise (ValueError if rc == -1 else RuntimeError)(f"gcs_keypoint_desc_ctx_create failed ({rc})")
        self.h, self.device = h, int(device)

    def close(self):
        if getattr(self, "h", None):
            self.lib.gcs_keypoint_desc_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc != 0:
            msg = self.lib.gcs_keypoint_desc_last_error(self.h).decode(errors="replace")
            raise (ValueError if rc in (-1, -3) else RuntimeError)(f"{what} failed ({rc}): {msg}")

    def _rows(self, x, dtype, n, what):
        import torch
        dev = torch.device(f"cuda:{self.device}")
        if not torch.is_tensor(x):
            x = torch.from_numpy(np.array(x, {torch.float32: np.float32, torch.int32: np.int32}[dtype]))   # (a copy: x may be read-only)
        if x.dtype != dtype or x.dim() != 1 or (n is not None and x.shape[0] != n):
            raise ValueError(f"{what}: {tuple(x.shape)} {x.dtype}, expected ({n},) {dtype}")
        return x.to(dev).contiguous()

    def queue(self, image, u, v, level=None) -> Descriptors:
        """gcs_describe_keypoints on the current torch stream, without waiting for anything: one row per entry of
        u, padding rows included (they come out invalid).  u, v: float32, level: int32 or None (level 0); device
        tensors are taken as they are, numpy arrays are uploaded."""
        import torch
        dev = torch.device(f"cuda:{self.device}")
        x, H, W, ch = self._image(image)
        u = self._rows(u, torch.float32, None, "u")
        n = int(u.shape[0])
        v = self._rows(v, torch.float32, n, "v")
        level = None if level is None else self._rows(level, torch.int32, n, "level")
        desc = torch.empty((n, DESC_BYTES), dtype=torch.uint8, device=dev)
        angle = torch.empty(n, dtype=torch.float32, device=dev)
        angle_bin = torch.empty(n, dtype=torch.int32, device=dev)
        i = KP._inputs_struct(x.data_ptr(), ch, x.stride(0), W, H)
        k = L.GcsKeypointDescKeypoints(n, u.data_ptr(), v.data_ptr(), None if level is None else level.data_ptr())
        o = L.GcsKeypointDescOutputs(angle.data_ptr(), angle_bin.data_ptr(), desc.data_ptr())
        self._chk(self.lib.gcs_keypoint_desc_ctx_set_stream(self.h, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
                  "gcs_keypoint_desc_ctx_set_stream")
        self._chk(self.lib.gcs_describe_keypoints(self.h, C.byref(i), C.byref(k), C.byref(o)), "gcs_describe_keypoints")
        return Descriptors(desc, angle, angle_bin)

    def describe(self, image, keypoints) -> Descriptors:
        """The descriptors of a Keypoints / PyramidKeypoints result (or a (u, v, response[, level]) tuple), device
        to device.  The row count is the keypoints' own, so the call waits for nothing."""
        u, v, level = _keypoint_arrays(keypoints)
        return self.queue(image, u, v, level)


_describers = {}


def _describer_for(config: DescriptorConfig, device: int, height: int, width: int, n: int) -> KeypointDescriber:
    """The cached describer of (config, device); its capacity grows to the largest image and row count seen."""
    key = (replace(config, max_width=0, max_height=0, max_keypoints=0), int(device))
    d = _describers.get(key)
    if d is None or d.h is None or d.config.max_width < width or d.config.max_height < height or d.config.max_keypoints < n:
        have = d.config if d is not None else config
        if d is not None:
            d.close()
        d = _describers[key] = KeypointDescriber(
            replace(config, max_width=max(have.max_width, config.max_width, width),
                    max_height=max(have.max_height, config.max_height, height),
                    max_keypoints=max(have.max_keypoints, config.max_keypoints, n)), device)
    return d


def describe_keypoints(image, keypoints, config: Optional[DescriptorConfig] = None, device: int = 0) -> Descriptors:
    """KeypointDescriber.describe on a cached describer of (config, device)."""
    H, W, _ = KP._shape(image.shape)
    n = int(tuple(keypoints)[0].shape[0])
    return _describer_for(config or DescriptorConfig(), device, H, W, n).describe(image, keypoints)


def describe_keypoints_host(image, keypoints, config: Optional[DescriptorConfig] = None, pitch: Optional[int] = None,
                            shape=None) -> Descriptors:
    """The same steps through gcs_describe_keypoints_host: numpy in and out, no device.  image, pitch and shape as
    gcslam.keypoints.detect_keypoints_host's."""
    config = config or DescriptorConfig()
    a = np.ascontiguousarray(image, np.uint8)
    if pitch is None:
        H, W, ch = KP._shape(a.shape)
        pitch = W * ch
    else:
        H, W, ch = (int(x) for x in shape)
        if a.ndim != 1 or H < 1 or a.size < (H - 1) * pitch + W * ch:
            raise ValueError("image: a flat buffer of at least (H - 1) * pitch + W * channels bytes")
    u, v, level = _keypoint_arrays(keypoints)
    u, v = np.ascontiguousarray(u, np.float32), np.ascontiguousarray(v, np.float32)
    n = int(u.shape[0])
    level = None if level is None else np.ascontiguousarray(level, np.int32)
    if u.ndim != 1 or v.shape != (n,) or (level is not None and level.shape != (n,)):
        raise ValueError("keypoints: u, v and level of one length")
    c = config_struct(replace(config, max_width=max(config.max_width, W), max_height=max(config.max_height, H),
                              max_keypoints=max(config.max_keypoints, n)), 0)
    desc, angle, angle_bin = np.empty((n, DESC_BYTES), np.uint8), np.empty(n, np.float32), np.empty(n, np.int32)
    i = KP._inputs_struct(a.ctypes.data, ch, pitch, W, H)
    k = L.GcsKeypointDescKeypoints(n, u.ctypes.data, v.ctypes.data, None if level is None else level.ctypes.data)
    o = L.GcsKeypointDescOutputs(angle.ctypes.data, angle_bin.ctypes.data, desc.ctypes.data)
    rc = L.load().gcs_describe_keypoints_host(C.byref(c), C.byref(i), C.byref(k), C.byref(o))
    if rc != 0:
        raise ValueError(f"gcs_describe_keypoints_host failed ({rc})")
    return Descriptors(desc, angle, angle_bin)


# ---- the matcher

@dataclass(frozen=True)
class MatchConfig:
    """gcs_match_config: the most query and train rows of a call."""
    max_query: int = 4096
    max_train: int = 4096


def match_config_struct(config: Optional[MatchConfig] = None, device: int = 0) -> "L.GcsMatchConfig":
    config = config or MatchConfig()
    c = L.GcsMatchConfig()
    L.check(L.load().gcs_match_config_defaults(C.byref(c)), None, "gcs_match_config_defaults")
    c.max_query, c.max_train, c.device = int(config.max_query), int(config.max_train), int(device)
    return c


@dataclass(frozen=True)
class GateConfig:
    """D8's window: radius in level-0 pixels around the predicted position, and the most levels apart."""
    radius: float = 16.0
    max_level_diff: int = 1


def gate_defaults() -> GateConfig:
    """gcs_match_gate_defaults as a GateConfig."""
    g = L.GcsMatchGate()
    L.check(L.load().gcs_match_gate_defaults(C.byref(g)), None, "gcs_match_gate_defaults")
    return GateConfig(float(g.radius), int(g.max_level_diff))


def filter_defaults():
    """gcs_match_filter_defaults: (max_distance, (ratio_num, ratio_den), cross_check)."""
    f = L.GcsMatchFilter()
    L.check(L.load().gcs_match_filter_defaults(C.byref(f)), None, "gcs_match_filter_defaults")
    return int(f.max_distance), (int(f.ratio_num), int(f.ratio_den)), bool(f.cross_check)


def _gate_struct(gate: GateConfig, pointers) -> "L.GcsMatchGate":
    """gcs_match_gate of q_u, q_v, q_level, t_u, t_v, t_level, q_pu, q_pv (addresses or None) and a GateConfig."""
    return L.GcsMatchGate(*pointers, float(gate.radius), int(gate.max_level_diff))


def _filter_struct(max_distance, ratio, cross_check) -> "L.GcsMatchFilter":
    """gcs_match_filter of match_descriptors' arguments: None switches a filter off (D9)."""
    num, den = (4, 0) if ratio is None else (int(r) for r in ratio)
    if ratio is not None and den == 0:
        raise ValueError("ratio: a denominator of 0")
    far = 256 if max_distance is None else max(-1, min(256, int(max_distance)))   # (no distance is below 0 or above 256)
    return L.GcsMatchFilter(far, num, den, 1 if cross_check else 0)


def _sides(a):
    """(desc, angle_bin or None) of a Descriptors object or of a bare (n, 32) uint8 array."""
    if isinstance(a, Descriptors):
        return a.desc, a.angle_bin
    return a, None


class DescriptorMatcher:
    """A gcs_match_ctx: the workspace of the train split for up to config.max_query x config.max_train rows."""

    def __init__(self, config: Optional[MatchConfig] = None, device: int = 0):
        self.config = config or MatchConfig()
        self.lib = L.load()
        c = match_config_struct(self.config, device)
        h = C.c_void_p()
        rc = self.lib.gcs_match_ctx_create(C.byref(c), C.byref(h))
        if rc != 0:
            raise (ValueError if rc == -1 else RuntimeError)(f"gcs_match_ctx_create failed ({rc})")
        self.h, self.device = h, int(device)

    def close(self):
        if getattr(self, "h", None):
            self.lib.gcs_match_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc != 0:
            msg = self.lib.gcs_match_last_error(self.h).decode(errors="replace")
            raise (ValueError if rc in (-1, -3) else RuntimeError)(f"{what} failed ({rc}): {msg}")

    def _desc(self, x, what):
        import torch
        dev = torch.device(f"cuda:{self.device}")
        if not torch.is_tensor(x):
            x = torch.from_numpy(np.array(x, np.uint8))
        if x.dtype != torch.uint8 or x.dim() != 2 or x.shape[1] != DESC_BYTES:
            raise ValueError(f"{what}: {tuple(x.shape)} {x.dtype}, expected (n, 32) uint8")
        x = x.to(dev).contiguous()
        return x if x.data_ptr() % 4 == 0 else x.clone()

    def _bins(self, x, n, what):
        import torch
        if x is None:
            return None
        if not torch.is_tensor(x):
            x = torch.from_numpy(np.array(x, np.int32))
        if x.dtype != torch.int32 or tuple(x.shape) != (n,):
            raise ValueError(f"{what}: {tuple(x.shape)} {x.dtype}, expected ({n},) int32")
        return x.to(torch.device(f"cuda:{self.device}")).contiguous()

    def queue(self, q, t, q_bin=None, t_bin=None):
        """gcs_match_descriptors on the current torch stream, without waiting: (idx, dist, dist2), int32 device
        tensors of one entry per query row (D7).  q, t: (n, 32) uint8; q_bin, t_bin: int32 or None."""
        import torch
        dev = torch.device(f"cuda:{self.device}")
        q, t = self._desc(q, "q"), self._desc(t, "t")
        n_q, n_t = int(q.shape[0]), int(t.shape[0])
        q_bin, t_bin = self._bins(q_bin, n_q, "q_bin"), self._bins(t_bin, n_t, "t_bin")
        out = torch.empty((3, n_q), dtype=torch.int32, device=dev)
        i = L.GcsMatchInputs(n_q, n_t, q.data_ptr() if n_q else None, t.data_ptr() if n_t else None,
                             None if q_bin is None or not n_q else q_bin.data_ptr(),
                             None if t_bin is None or not n_t else t_bin.data_ptr())
        o = L.GcsMatchOutputs(*((out[j].data_ptr() if n_q else None) for j in range(3)))
        self._chk(self.lib.gcs_match_ctx_set_stream(self.h, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
                  "gcs_match_ctx_set_stream")
        self._chk(self.lib.gcs_match_descriptors(self.h, C.byref(i), C.byref(o)), "gcs_match_descriptors")
        return out[0], out[1], out[2]

    def _positions(self, kp, n, what):
        """(u, v, level or None) of one side as device tensors of n rows."""
        import torch
        u, v, level = _keypoint_arrays(kp)
        return (KeypointDescriber._rows(self, u, torch.float32, n, what + " u"),
                KeypointDescriber._rows(self, v, torch.float32, n, what + " v"),
                None if level is None else KeypointDescriber._rows(self, level, torch.int32, n, what + " level"))

    def _gate(self, kp_q, kp_t, predicted, gate, n_q, n_t):
        """(gcs_match_gate, the tensors it points into) of device positions."""
        import torch
        gate = gate or GateConfig()
        q, t = self._positions(kp_q, n_q, "kp_q"), self._positions(kp_t, n_t, "kp_t")
        p = (None, None)
        if predicted is not None:
            pu, pv = tuple(predicted)[:2]
            p = (KeypointDescriber._rows(self, pu, torch.float32, n_q, "predicted u"),
                 KeypointDescriber._rows(self, pv, torch.float32, n_q, "predicted v"))
        g = _gate_struct(gate, [None if x is None or not x.shape[0] else x.data_ptr() for x in q + t + p])
        return g, (q, t, p)

    def _inputs(self, q, t, q_bin, t_bin):
        q, t = self._desc(q, "q"), self._desc(t, "t")
        n_q, n_t = int(q.shape[0]), int(t.shape[0])
        q_bin, t_bin = self._bins(q_bin, n_q, "q_bin"), self._bins(t_bin, n_t, "t_bin")
        i = L.GcsMatchInputs(n_q, n_t, q.data_ptr() if n_q else None, t.data_ptr() if n_t else None,
                             None if q_bin is None or not n_q else q_bin.data_ptr(),
                             None if t_bin is None or not n_t else t_bin.data_ptr())
        return i, n_q, n_t, (q, t, q_bin, t_bin)

    def queue_gated(self, q, t, kp_q, kp_t, predicted=None, gate: Optional["GateConfig"] = None, q_bin=None, t_bin=None):
        """gcs_match_descriptors_gated on the current torch stream, without waiting: (idx, dist, dist2, n_cand), int32
        device tensors of one entry per query row (D8).  kp_q, kp_t: a detector's result or a (u, v[, response[,
        level]]) tuple; predicted: (pu, pv) of every query row, or None (the query's own position); gate: a
        GateConfig (None: its defaults)."""
        import torch
        dev = torch.device(f"cuda:{self.device}")
        i, n_q, n_t, keep = self._inputs(q, t, q_bin, t_bin)
        g, keep_g = self._gate(kp_q, kp_t, predicted, gate, n_q, n_t)
        out = torch.empty((4, n_q), dtype=torch.int32, device=dev)
        o = L.GcsMatchGatedOutputs(*((out[j].data_ptr() if n_q else None) for j in range(4)))
        self._chk(self.lib.gcs_match_ctx_set_stream(self.h, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
                  "gcs_match_ctx_set_stream")
        self._chk(self.lib.gcs_match_descriptors_gated(self.h, C.byref(i), C.byref(g), C.byref(o)), "gcs_match_descriptors_gated")
        return out[0], out[1], out[2], out[3]

    def queue_pairs(self, q, t, kp_q=None, kp_t=None, predicted=None, gate: Optional["GateConfig"] = None, q_bin=None,
                    t_bin=None, max_distance: Optional[int] = 64, ratio=(4, 5), cross_check: bool = True):
        """gcs_match_pairs on the current torch stream, without waiting: the padded (pair_a, pair_b, pair_dist) of
        n_query entries each and count, a one-entry tensor, all int32 on the device (D9).  Without kp_q and kp_t
        there is no gate."""
        import torch
        dev = torch.device(f"cuda:{self.device}")
        i, n_q, n_t, keep = self._inputs(q, t, q_bin, t_bin)
        g = None
        if kp_q is not None or kp_t is not None or gate is not None:
            if kp_q is None or kp_t is None:
                raise ValueError("a gate needs both kp_q and kp_t")
            g, keep_g = self._gate(kp_q, kp_t, predicted, gate, n_q, n_t)
        f = _filter_struct(max_distance, ratio, cross_check)
        out = torch.empty((3, n_q), dtype=torch.int32, device=dev)
        count = torch.empty(1, dtype=torch.int32, device=dev)
        o = L.GcsMatchPairOutputs(*((out[j].data_ptr() if n_q else None) for j in range(3)), count.data_ptr())
        self._chk(self.lib.gcs_match_ctx_set_stream(self.h, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
                  "gcs_match_ctx_set_stream")
        self._chk(self.lib.gcs_match_pairs(self.h, C.byref(i), None if g is None else C.byref(g), C.byref(f), C.byref(o)),
                  "gcs_match_pairs")
        return out[0], out[1], out[2], count


_matchers = {}


def _matcher_for(device: int, n_q: int, n_t: int) -> DescriptorMatcher:
    """The cached matcher of a device; its capacity grows to the largest sets seen."""
    m = _matchers.get(int(device))
    if m is None or m.h is None or m.config.max_query < n_q or m.config.max_train < n_t:
        have = m.config if m is not None else MatchConfig()
        if m is not None:
            m.close()
        m = _matchers[int(device)] = DescriptorMatcher(MatchConfig(max(have.max_query, n_q), max(have.max_train, n_t)), device)
    return m


def _filters(idx, dist, dist2, max_distance, ratio):
    keep = idx >= 0
    if max_distance is not None:
        keep = keep & (dist <= int(max_distance))
    if ratio is not None:
        num, den = (int(r) for r in ratio)
        keep = keep & (dist * den < num * dist2)
    return keep


def match_descriptors(a, b, max_distance: Optional[int] = 64, ratio=(4, 5), cross_check: bool = True, device: int = 0):
    """Matches of two descriptor sets: (idx_a, idx_b, dist), int device tensors in ascending idx_a.  a, b:
    Descriptors (invalid rows are left out through .angle_bin) or bare (n, 32) uint8 arrays.  The kernel gives
    every row of a its nearest and second-nearest row of b (and, with cross_check, the same the other way); the
    filters are integer torch ops on the device: dist <= max_distance, dist * den < num * dist2 with ratio =
    (num, den), and b's nearest row of a being the row itself.  The defaults of the three filters are conveniences
    of this function, not part of the operator's definition; None switches the first two off.  Building the
    result's length waits for the device once."""
    import torch
    qa, ba = _sides(a)
    qb, bb = _sides(b)
    n_a, n_b = int(qa.shape[0]), int(qb.shape[0])
    m = _matcher_for(device, max(n_a, n_b), max(n_a, n_b)) if cross_check else _matcher_for(device, n_a, n_b)
    idx, dist, dist2 = m.queue(qa, qb, ba, bb)
    keep = _filters(idx, dist, dist2, max_distance, ratio)
    if cross_check:
        back = m.queue(qb, qa, bb, ba)[0]
        if back.shape[0]:
            rows = torch.arange(idx.shape[0], dtype=torch.int32, device=idx.device)
            keep = keep & (back[idx.clamp(min=0).long()] == rows)
        else:
            keep = keep & False
    at = torch.nonzero(keep).flatten()
    return at.to(torch.int32), idx[at], dist[at]


def nearest_host(q, t, q_bin=None, t_bin=None):
    """gcs_match_descriptors_host: (idx, dist, dist2) int32 numpy arrays of one entry per row of q (D7)."""
    q, t = np.ascontiguousarray(q, np.uint8), np.ascontiguousarray(t, np.uint8)
    for x, what in ((q, "q"), (t, "t")):
        if x.ndim != 2 or x.shape[1] != DESC_BYTES:
            raise ValueError(f"{what}: {x.shape}, expected (n, 32) uint8")
    n_q, n_t = q.shape[0], t.shape[0]
    q_bin = None if q_bin is None else np.ascontiguousarray(q_bin, np.int32)
    t_bin = None if t_bin is None else np.ascontiguousarray(t_bin, np.int32)
    if (q_bin is not None and q_bin.shape != (n_q,)) or (t_bin is not None and t_bin.shape != (n_t,)):
        raise ValueError("q_bin, t_bin: one entry per row")
    c = match_config_struct(MatchConfig(max(n_q, 1), max(n_t, 1)), 0)
    out = np.empty((3, n_q), np.int32)
    i = L.GcsMatchInputs(n_q, n_t, q.ctypes.data if n_q else None, t.ctypes.data if n_t else None,
                         None if q_bin is None or not n_q else q_bin.ctypes.data,
                         None if t_bin is None or not n_t else t_bin.ctypes.data)
    o = L.GcsMatchOutputs(*((out[j].ctypes.data if n_q else None) for j in range(3)))
    rc = L.load().gcs_match_descriptors_host(C.byref(c), C.byref(i), C.byref(o))
    if rc != 0:
        raise ValueError(f"gcs_match_descriptors_host failed ({rc})")
    return out[0], out[1], out[2]


def match_descriptors_host(a, b, max_distance: Optional[int] = 64, ratio=(4, 5), cross_check: bool = True):
    """match_descriptors through gcs_match_descriptors_host and numpy: no device."""
    qa, ba = _sides(a)
    qb, bb = _sides(b)
    idx, dist, dist2 = nearest_host(qa, qb, ba, bb)
    keep = _filters(idx, dist.astype(np.int64), dist2.astype(np.int64), max_distance, ratio)
    if cross_check:
        back = nearest_host(qb, qa, bb, ba)[0]
        keep = keep & (back[np.clip(idx, 0, None)] == np.arange(len(idx))) if len(back) else keep & False
    at = np.nonzero(keep)[0]
    return at.astype(np.int32), idx[at], dist[at]


# ---- the gate and the pairs (D8, D9)

def match_pairs(a, b, kp_a=None, kp_b=None, predicted=None, gate: Optional[GateConfig] = None,
                max_distance: Optional[int] = 64, ratio=(4, 5), cross_check: bool = True, device: int = 0):
    """match_descriptors' triple (idx_a, idx_b, dist) through gcs_match_pairs: both searches, the filters, the cross
    check and the compaction in one device pass, cut to the count -- one wait, for its 4 bytes.  With kp_a and kp_b
    (detector results or (u, v[, response[, level]]) tuples) a row of b is a candidate only inside the window of
    `gate` (None: GateConfig()) around `predicted` = (pu, pv), where each row of a is expected in b's image (None:
    the row's own position).  Passing gate without both kp_a and kp_b raises ValueError."""
    import torch
    if (gate is not None or predicted is not None) and (kp_a is None or kp_b is None):
        raise ValueError("a gate needs both kp_a and kp_b")
    qa, ba = _sides(a)
    qb, bb = _sides(b)
    m = _matcher_for(device, int(qa.shape[0]), int(qb.shape[0]))
    pa, pb, pd, count = m.queue_pairs(qa, qb, kp_a, kp_b, predicted, gate, ba, bb, max_distance, ratio, cross_check)
    n = int(count.item())
    return pa[:n], pb[:n], pd[:n]


def _host_inputs(q, t, q_bin, t_bin):
    q, t = np.ascontiguousarray(q, np.uint8), np.ascontiguousarray(t, np.uint8)
    for x, what in ((q, "q"), (t, "t")):
        if x.ndim != 2 or x.shape[1] != DESC_BYTES:
            raise ValueError(f"{what}: {x.shape}, expected (n, 32) uint8")
    n_q, n_t = q.shape[0], t.shape[0]
    q_bin = None if q_bin is None else np.ascontiguousarray(q_bin, np.int32)
    t_bin = None if t_bin is None else np.ascontiguousarray(t_bin, np.int32)
    if (q_bin is not None and q_bin.shape != (n_q,)) or (t_bin is not None and t_bin.shape != (n_t,)):
        raise ValueError("q_bin, t_bin: one entry per row")
    i = L.GcsMatchInputs(n_q, n_t, q.ctypes.data if n_q else None, t.ctypes.data if n_t else None,
                         None if q_bin is None or not n_q else q_bin.ctypes.data,
                         None if t_bin is None or not n_t else t_bin.ctypes.data)
    return i, n_q, n_t, (q, t, q_bin, t_bin)


def _host_gate(kp_q, kp_t, predicted, gate, n_q, n_t):
    rows = []
    for kp, n in ((kp_q, n_q), (kp_t, n_t)):
        u, v, level = _keypoint_arrays(kp)
        rows += [np.ascontiguousarray(u, np.float32), np.ascontiguousarray(v, np.float32),
                 None if level is None else np.ascontiguousarray(level, np.int32)]
        if any(x is not None and x.shape != (n,) for x in rows[-3:]):
            raise ValueError("keypoints: u, v and level of one entry per descriptor row")
    if predicted is None:
        rows += [None, None]
    else:
        rows += [np.ascontiguousarray(x, np.float32) for x in tuple(predicted)[:2]]
        if any(x.shape != (n_q,) for x in rows[-2:]):
            raise ValueError("predicted: (pu, pv) of one entry per query row")
    return _gate_struct(gate or GateConfig(), [None if x is None or not x.shape[0] else x.ctypes.data for x in rows]), rows


def nearest_gated_host(q, t, kp_q, kp_t, predicted=None, gate: Optional[GateConfig] = None, q_bin=None, t_bin=None):
    """gcs_match_descriptors_gated_host: (idx, dist, dist2, n_cand) int32 numpy arrays of one entry per row of q (D8)."""
    i, n_q, n_t, keep = _host_inputs(q, t, q_bin, t_bin)
    g, keep_g = _host_gate(kp_q, kp_t, predicted, gate, n_q, n_t)
    c = match_config_struct(MatchConfig(max(n_q, 1), max(n_t, 1)), 0)
    out = np.empty((4, n_q), np.int32)
    o = L.GcsMatchGatedOutputs(*((out[j].ctypes.data if n_q else None) for j in range(4)))
    rc = L.load().gcs_match_descriptors_gated_host(C.byref(c), C.byref(i), C.byref(g), C.byref(o))
    if rc != 0:
        raise ValueError(f"gcs_match_descriptors_gated_host failed ({rc})")
    return out[0], out[1], out[2], out[3]


def pairs_host(q, t, kp_q=None, kp_t=None, predicted=None, gate: Optional[GateConfig] = None, q_bin=None, t_bin=None,
               max_distance: Optional[int] = 64, ratio=(4, 5), cross_check: bool = True):
    """gcs_match_pairs_host: the padded (pair_a, pair_b, pair_dist) and the count, as DescriptorMatcher.queue_pairs."""
    i, n_q, n_t, keep = _host_inputs(q, t, q_bin, t_bin)
    g = None
    if kp_q is not None or kp_t is not None or gate is not None or predicted is not None:
        if kp_q is None or kp_t is None:
            raise ValueError("a gate needs both kp_q and kp_t")
        g, keep_g = _host_gate(kp_q, kp_t, predicted, gate, n_q, n_t)
    f = _filter_struct(max_distance, ratio, cross_check)
    c = match_config_struct(MatchConfig(max(n_q, 1), max(n_t, 1)), 0)
    out, count = np.empty((3, n_q), np.int32), np.full(1, -7, np.int32)
    o = L.GcsMatchPairOutputs(*((out[j].ctypes.data if n_q else None) for j in range(3)), count.ctypes.data)
    rc = L.load().gcs_match_pairs_host(C.byref(c), C.byref(i), None if g is None else C.byref(g), C.byref(f), C.byref(o))
    if rc != 0:
        raise ValueError(f"gcs_match_pairs_host failed ({rc})")
    return out[0], out[1], out[2], count


def match_pairs_host(a, b, kp_a=None, kp_b=None, predicted=None, gate: Optional[GateConfig] = None,
                     max_distance: Optional[int] = 64, ratio=(4, 5), cross_check: bool = True):
    """match_pairs through gcs_match_pairs_host: numpy in and out, no device."""
    qa, ba = _sides(a)
    qb, bb = _sides(b)
    pa, pb, pd, count = pairs_host(qa, qb, kp_a, kp_b, predicted, gate, ba, bb, max_distance, ratio, cross_check)
    n = int(count[0])
    return pa[:n], pb[:n], pd[:n]
