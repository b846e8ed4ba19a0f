"""Rendering the primitive map on the MI355X: the reference's output side -- the BEV pushforward of 3-D
Gaussians (FS/common/bev_pushforward.py), opacity from precision, multi-lobe vMF shading, world-space
fBm, tile binning with a fixed cap and tiled EWA rendering (FS/backend/rendering.py) -- with the
reference's names and config dataclasses, batched over device tensors.

  oblique_Ps_bev15                bev_pushforward.py:72-88   host
  pushforward_gaussians_3d_to_2d  :42-64                     (N,3), (N,3,3), (V,2,3) -> (V,N,2), (V,N,2,2)
  rotate_vmf_etas                 :103-109
  opacity_from_logdet             rendering.py:236-244
  vmf_shading_multi_lobe          :117-159                   one view direction against (N,B,3) lobes
  fbm_at_splat_positions          :167-228
  splat_indices_for_tiles         :252-289                   every tile of every view  (gcs_render_bin_tiles)
  render_tiles_ewa                :297-355                   every tile of every view  (gcs_render_tiles)
  render_map_view                 the composed call: an AtlasMapView (or an AtlasMap and tile ids) to
                                  (V,H,W,3) images in one library call             (gcs_render_view)

The five per-element operators are a few tensor expressions each (f64, the reference's operation order,
integer hash in int64); binning, tile rendering and the composed call's per-row math are HIP kernels
(csrc/gcs_render.hip), and without the library they raise: there is no other route.  The reference has
no driver for the whole chain; the composition render_map_view declares is DESIGN.md section 3.
"""

from __future__ import annotations

import ctypes as C
from collections import OrderedDict
from dataclasses import astuple, dataclass
from typing import Optional

import numpy as np

from . import _lib as L


@dataclass(frozen=True)
class SplatRenderingConfig:
    """rendering.py:28-44: same fields and defaults."""
    tile_size: int = 32
    max_splats_per_tile: int = 64
    fbm_octaves: int = 5
    fbm_gain: float = 0.5
    opacity_gamma: float = 1.0
    logdet0: float = 0.0
    eps: float = 1e-12
    ewa_log_clip: float = 25.0
    alpha_min: float = 0.02
    vmf_intensity_scale: float = 0.5
    vmf_intensity_max: float = 255.0
    vmf_kappa_max: float = 100.0


@dataclass(frozen=True)
class BEVPushforwardConfig:
    """bev_pushforward.py:16-27: same fields and defaults."""
    oblique_phi_deg: float = 10.0
    n_views: int = 15
    phi_center_deg: float = 10.0
    phi_span_deg: float = 14.0


@dataclass
class RenderResult:
    images: object          # (V, H, W, 3) f64
    tile_indices: object    # (V, Ty, Tx, max_splats_per_tile) int32, view rows, padded with -1
    tile_counts: object     # (V, Ty, Tx) int32
    splats: Optional[dict] = None   # the 2-D record (means, Sigmas_inv, radii, alphas, colors, fbm) when asked for


def _torch():
    import torch
    return torch


def _dev(x, dtype=None, device=None):
    torch = _torch()
    dtype = dtype or torch.float64
    if isinstance(x, torch.Tensor):
        return x.to(dtype=dtype).contiguous() if device is None else x.to(device=device, dtype=dtype).contiguous()
    return torch.tensor(np.asarray(x), dtype=dtype, device=device or "cuda:0").contiguous()


# ---------------------------------------------------------------------- views
def bev15_phis_deg(config: BEVPushforwardConfig) -> np.ndarray:
    """The oblique angles of oblique_Ps_bev15's views (degrees)."""
    n = max(1, int(config.n_views))
    if n == 1:
        return np.array([float(config.phi_center_deg)], dtype=np.float64)
    return float(config.phi_center_deg) + np.linspace(-0.5, 0.5, n, dtype=np.float64) * float(config.phi_span_deg)


def oblique_Ps_bev15(config: BEVPushforwardConfig = BEVPushforwardConfig()) -> np.ndarray:
    """(V, 2, 3) host array: P(phi) = [[1, 0, 0], [0, cos phi, sin phi]] along the sweep."""
    phis = np.deg2rad(bev15_phis_deg(config))
    Ps = np.zeros((phis.shape[0], 2, 3), dtype=np.float64)
    Ps[:, 0, 0] = 1.0
    Ps[:, 1, 1] = np.cos(phis)
    Ps[:, 1, 2] = np.sin(phis)
    return Ps


def view_geometry(bev: BEVPushforwardConfig, width: int, height: int, pixels_per_metre: float, centre_xy):
    """The composed call's per-view host arrays: P_pix = s P(phi_k) (V, 2, 3), the offsets
    b = (W/2, H/2) - P_pix (cx, cy, 0) (V, 2) and the view directions (0, sin phi_k, -cos phi_k) (V, 3)."""
    P_pix = float(pixels_per_metre) * oblique_Ps_bev15(bev)
    c = np.array([float(centre_xy[0]), float(centre_xy[1]), 0.0])
    offsets = np.array([0.5 * width, 0.5 * height]) - P_pix @ c
    phis = np.deg2rad(bev15_phis_deg(bev))
    view_dirs = np.stack([np.zeros_like(phis), np.sin(phis), -np.cos(phis)], axis=1)
    return P_pix, offsets, view_dirs


# ---------------------------------------------------------------------- per-element operators
def pushforward_gaussians_3d_to_2d(mu, Sigma, P):
    """mu' = P mu, Sigma' = P Sigma P^T for every (view, row): (V, N, 2) and (V, N, 2, 2)."""
    mu, Sigma = _dev(mu).reshape(-1, 3), _dev(Sigma).reshape(-1, 3, 3)
    P = _dev(P, device=mu.device).reshape(-1, 2, 3)
    Pv, m = P[:, None], mu[None, :, None, :]                                    # (V, 1, 2, 3), (1, N, 1, 3)
    mu2 = (Pv[..., 0] * m[..., 0] + Pv[..., 1] * m[..., 1]) + Pv[..., 2] * m[..., 2]
    Pc, Sg = P[:, None, :, :, None], Sigma[None, :, None, :, :]                 # sums left to right, no reduction
    PS = (Pc[..., 0, :] * Sg[..., 0, :] + Pc[..., 1, :] * Sg[..., 1, :]) + Pc[..., 2, :] * Sg[..., 2, :]   # (V, N, 2, 3)
    Pr, Q = P[:, None, None, :, :], PS[:, :, :, None, :]
    S2 = (Q[..., 0] * Pr[..., 0] + Q[..., 1] * Pr[..., 1]) + Q[..., 2] * Pr[..., 2]   # (V, N, 2, 2)
    return mu2, S2


def rotate_vmf_etas(R, etas):
    """eta' = R eta for (..., 3) natural parameters."""
    etas = _dev(etas)
    R = _dev(R, device=etas.device).reshape(3, 3)
    e = etas[..., None, :]
    return (e[..., 0] * R[:, 0] + e[..., 1] * R[:, 1]) + e[..., 2] * R[:, 2]


def opacity_from_logdet(logdet_cov, gamma: float = 1.0, logdet0: float = 0.0, alpha_min: float = 0.02):
    """alpha = alpha_min + (1 - alpha_min) sigma(gamma (logdet0 - logdet))."""
    torch = _torch()
    raw = 1.0 / (1.0 + torch.exp(-float(gamma) * (float(logdet0) - _dev(logdet_cov))))
    return float(alpha_min) + (1.0 - float(alpha_min)) * raw


def vmf_shading_multi_lobe(v, mu_app, kappa_app, pi_b=None, intensity=None, intensity_scale: float = 0.0,
                           intensity_max: float = 255.0, kappa_max: float = 100.0, eps: float = 1e-12):
    """s = sum_b pi_b exp(kappa_b (mu_b . v - 1)) / (1 + mean kappa) for N rows of B lobes: mu_app (N, B, 3),
    kappa_app (N, B); pi_b (B,) or (N, B), default uniform; intensity (N,), (N, B) or a scalar.  Returns
    (N,).  The inputs are left as they are (the reference normalises mu_app in place)."""
    torch = _torch()
    mu = _dev(mu_app)
    mu = mu.reshape(mu.shape[0], -1, 3)
    N, B = mu.shape[0], mu.shape[1]
    k = _dev(kappa_app, device=mu.device).reshape(N, B)
    v = _dev(v, device=mu.device).reshape(3)
    v = v / (torch.sqrt((v * v).sum()) + eps)
    mu = mu / (torch.sqrt((mu * mu).sum(-1, keepdim=True)) + eps)
    if pi_b is None:
        pi = torch.full((N, B), 1.0 / B, dtype=torch.float64, device=mu.device)
    else:
        pi = _dev(pi_b, device=mu.device).reshape(-1, B).expand(N, B)
        pi = pi / (pi.sum(-1, keepdim=True) + eps)
    if intensity_scale > 0.0 and intensity is not None and intensity_max > eps:
        t = _dev(intensity, device=mu.device)
        t = t.reshape(N, -1) if t.numel() >= N and t.numel() > 1 else t.reshape(1, 1)
        t = torch.clamp(t / max(float(intensity_max), eps), 0.0, 1.0)
        k = torch.clamp(k * (1.0 + float(intensity_scale) * t), max=float(kappa_max))
    s = (pi * torch.exp(k * ((mu * v).sum(-1) - 1.0))).sum(-1)
    return s / (1.0 + k.sum(-1) / max(B, 1))


def _hash_float(h):
    h = (h * 1103515245 + 12345) & 0x7FFFFFFF
    return h.to(_torch().float64) / 2147483648.0


def _value_noise_2d(x, y, seed: int):
    torch = _torch()
    flx, fly = torch.floor(x), torch.floor(y)
    ix, iy = flx.to(torch.int64), fly.to(torch.int64)
    fx, fy = torch.clamp(x - flx, 0.0, 1.0), torch.clamp(y - fly, 0.0, 1.0)
    s31 = int(seed) * 31
    v00 = _hash_float(((s31 + ix) * 31 + iy) & 0x7FFFFFFF)
    v10 = _hash_float(((s31 + ix + 1) * 31 + iy) & 0x7FFFFFFF)
    v01 = _hash_float(((s31 + ix) * 31 + iy + 1) & 0x7FFFFFFF)
    v11 = _hash_float(((s31 + ix + 1) * 31 + iy + 1) & 0x7FFFFFFF)
    sx, sy = fx * fx * (3.0 - 2.0 * fx), fy * fy * (3.0 - 2.0 * fy)
    v0 = v00 * (1 - sx) + v10 * sx
    v1 = v01 * (1 - sx) + v11 * sx
    return v0 * (1 - sy) + v1 * sy


def fbm_at_splat_positions(means_world_xy, octaves: int = 5, gain: float = 0.5, seed: int = 0):
    """fBm value noise at (N, 2) world positions: (N,) in [0, 1].  The hash runs in int64, whose wrap-around
    leaves the masked low 31 bits equal to Python's unbounded integers'."""
    torch = _torch()
    xy = _dev(means_world_xy).reshape(-1, 2)
    x, y = xy[:, 0], xy[:, 1]
    value = torch.zeros_like(x)
    amplitude, frequency, max_amplitude = 1.0, 1.0, 0.0
    for _ in range(int(octaves)):
        value = value + amplitude * _value_noise_2d(x * frequency, y * frequency, seed)
        max_amplitude += amplitude
        amplitude *= float(gain)
        frequency *= 2.0
    return value / (max_amplitude + 1e-12)


# ---------------------------------------------------------------------- the library side
def _config_struct(cfg: SplatRenderingConfig, device: int = 0) -> L.GcsRenderConfig:
    c = L.GcsRenderConfig()
    L.check(L.load().gcs_render_config_defaults(C.byref(c)), None, "gcs_render_config_defaults")
    for name, val in zip(cfg.__dataclass_fields__, astuple(cfg)):
        setattr(c, name, val)
    c.device = int(device)
    return c


def config_defaults() -> SplatRenderingConfig:
    """SplatRenderingConfig as gcs_render_config_defaults fills it."""
    c = L.GcsRenderConfig()
    L.check(L.load().gcs_render_config_defaults(C.byref(c)), None, "gcs_render_config_defaults")
    return SplatRenderingConfig(**{n: getattr(c, n) for n in SplatRenderingConfig.__dataclass_fields__})


def tile_grid(width: int, height: int, tile_size: int):
    """(tile, n_ty, n_tx) with the reference's clamp of the tile size to [1, 32]."""
    t = min(max(int(tile_size), 1), 32)
    return t, (int(height) + t - 1) // t, (int(width) + t - 1) // t


def _prepare_inputs(n_rows, n_views, rows, P_pix, offsets, view_dirs, fbm_modulate_scale, fbm_seed, ptr):
    """rows: name -> array (None allowed for valid_mask / intensity); ptr: array -> address."""
    i = L.GcsRenderPrepareInputs()
    i.n_rows, i.n_views = int(n_rows), int(n_views)
    for name in L.RENDER_ROW_FIELDS:
        x = rows.get(name)
        setattr(i, name, ptr(x) if x is not None and n_rows else None)
    keep = [np.ascontiguousarray(a, np.float64).reshape(n_views, w)
            for a, w in ((P_pix, 6), (offsets, 2), (view_dirs, 3))]
    for name, a in zip(L.RENDER_VIEW_FIELDS, keep):
        setattr(i, name, a.ctypes.data)
    i.fbm_modulate_scale, i.fbm_seed = float(fbm_modulate_scale), int(fbm_seed)
    return i, keep


def prepare_splats_host(positions, covariances, directions, kappas, colors, valid_mask, P_pix, offsets, view_dirs,
                        cfg: SplatRenderingConfig = SplatRenderingConfig(), fbm_modulate_scale: float = 0.0,
                        fbm_seed: int = 0, intensity=None) -> dict:
    """gcs_render_prepare_host: the prepare kernel's per-row math built for the host, on numpy arrays."""
    n = int(np.asarray(kappas).reshape(-1).shape[0])
    V = int(np.asarray(P_pix).reshape(-1, 6).shape[0])
    rows = {"positions": (positions, 3), "covariances": (covariances, 9), "directions": (directions, 3),
            "kappas": (kappas, 1), "colors": (colors, 3), "intensity": (intensity, 1)}
    rows = {k: None if a is None else np.ascontiguousarray(a, np.float64).reshape(n, w) for k, (a, w) in rows.items()}
    rows["valid_mask"] = None if valid_mask is None else np.ascontiguousarray(valid_mask).astype(np.uint8).reshape(n)
    i, keep = _prepare_inputs(n, V, rows, P_pix, offsets, view_dirs, fbm_modulate_scale, fbm_seed,
                              lambda a: a.ctypes.data)
    shapes = {"means": (V, n, 2), "Sigmas_inv": (V, n, 2, 2), "radii": (V, n), "alphas": (n,), "colors": (V, n, 3),
              "fbm": (n,)}
    out = {k: np.zeros(s) for k, s in shapes.items()}
    o = L.GcsRenderSplats()
    for k, a in out.items():
        setattr(o, k, a.ctypes.data if n else None)
    c = _config_struct(cfg)
    rc = L.load().gcs_render_prepare_host(C.byref(c), C.byref(i), C.byref(o))
    if rc != 0:
        raise ValueError(f"gcs_render_prepare_host failed ({rc})")
    return out


class Renderer:
    """A gcs_render_ctx: one SplatRenderingConfig on one GPU."""

    def __init__(self, cfg: SplatRenderingConfig = SplatRenderingConfig(), device: int = 0):
        self.lib = L.load()
        self.cfg, self.device = cfg, int(device)
        c = _config_struct(cfg, device)
        h = C.c_void_p()
        rc = self.lib.gcs_render_ctx_create(C.byref(c), C.byref(h))
        if rc != 0:
            raise (ValueError if rc == -1 else RuntimeError)(f"gcs_render_ctx_create failed ({rc}): {cfg}")
        self.h = h
        self.cap = int(cfg.max_splats_per_tile)

    def close(self):
        if getattr(self, "h", None):
            self.lib.gcs_render_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc != 0:
            msg = self.lib.gcs_render_last_error(self.h).decode(errors="replace")
            raise (ValueError if rc in (-1, -3) else RuntimeError)(f"{what} failed ({rc}): {msg}")

    @property
    def dev(self):
        return f"cuda:{self.device}"

    def _stream(self):
        """Hands torch's current stream to the context and drains it first: the uploads and conversions above
        were queued there, and a null-stream handle selects the context's own non-blocking stream, which the
        null stream does not order."""
        ts = _torch().cuda.current_stream(self.dev)
        self._chk(self.lib.gcs_render_ctx_set_stream(self.h, C.c_void_p(ts.cuda_stream)), "gcs_render_ctx_set_stream")
        ts.synchronize()

    def _splats(self, V, n):
        torch = _torch()
        shapes = {"means": (V, n, 2), "Sigmas_inv": (V, n, 2, 2), "radii": (V, n), "alphas": (n,),
                  "colors": (V, n, 3), "fbm": (n,)}
        # k_rn_prepare writes every element of the record (nothing to write when n = 0)
        t = {k: torch.empty(s, dtype=torch.float64, device=self.dev) for k, s in shapes.items()}
        o = L.GcsRenderSplats()
        for k, x in t.items():
            setattr(o, k, x.data_ptr() if n else None)
        return t, o

    def _tile_outputs(self, V, width, height):
        torch = _torch()
        _, n_ty, n_tx = tile_grid(width, height, self.cfg.tile_size)
        idx = torch.empty((V, n_ty, n_tx, self.cap), dtype=torch.int32, device=self.dev)
        cnt = torch.empty((V, n_ty, n_tx), dtype=torch.int32, device=self.dev)
        return idx, cnt

    def _rows(self, positions, covariances, directions, kappas, colors, valid_mask, intensity):
        torch = _torch()
        k = _dev(kappas, device=self.dev).reshape(-1)
        n = int(k.shape[0])
        rows = {"positions": _dev(positions, device=self.dev).reshape(n, 3),
                "covariances": _dev(covariances, device=self.dev).reshape(n, 9),
                "directions": _dev(directions, device=self.dev).reshape(n, 3), "kappas": k,
                "colors": _dev(colors, device=self.dev).reshape(n, 3),
                "valid_mask": None if valid_mask is None else
                _dev(valid_mask, torch.bool, self.dev).reshape(n).view(torch.uint8),
                "intensity": None if intensity is None else _dev(intensity, device=self.dev).reshape(n)}
        return n, rows

    def prepare(self, positions, covariances, directions, kappas, colors, valid_mask, P_pix, offsets, view_dirs,
                fbm_modulate_scale: float = 0.0, fbm_seed: int = 0, intensity=None) -> dict:
        """gcs_render_prepare: the 2-D record of every (view, row) as device tensors."""
        n, rows = self._rows(positions, covariances, directions, kappas, colors, valid_mask, intensity)
        V = int(np.asarray(P_pix).reshape(-1, 6).shape[0])
        i, keep = _prepare_inputs(n, V, rows, P_pix, offsets, view_dirs, fbm_modulate_scale, fbm_seed,
                                  lambda x: x.data_ptr())
        t, o = self._splats(V, n)
        self._stream()
        self._chk(self.lib.gcs_render_prepare(self.h, C.byref(i), C.byref(o)), "gcs_render_prepare")
        return t

    def bin_tiles(self, means, Sigmas_inv, width: int, height: int, radii=None):
        """gcs_render_bin_tiles: (indices (V, Ty, Tx, cap) int32, counts (V, Ty, Tx) int32)."""
        m = _dev(means, device=self.dev)
        V, n = int(m.shape[0]), int(m.shape[1])
        S = None if Sigmas_inv is None else _dev(Sigmas_inv, device=self.dev).reshape(V, n, 4)
        r = None if radii is None else _dev(radii, device=self.dev).reshape(V, n)
        idx, cnt = self._tile_outputs(V, width, height)
        p = lambda x: x.data_ptr() if x is not None and n else None   # noqa: E731
        self._stream()
        self._chk(self.lib.gcs_render_bin_tiles(self.h, V, n, int(width), int(height), p(m), p(r), p(S),
                                                idx.data_ptr(), cnt.data_ptr()), "gcs_render_bin_tiles")
        return idx, cnt

    def render_tiles(self, means, Sigmas_inv, alphas, colors, tile_indices, tile_counts, width: int, height: int,
                     image_layout: bool = False):
        """gcs_render_tiles: (V, Ty, Tx, tile, tile, 3), or (V, H, W, 3) with image_layout."""
        torch = _torch()
        m = _dev(means, device=self.dev)
        V, n = int(m.shape[0]), int(m.shape[1])
        S = _dev(Sigmas_inv, device=self.dev).reshape(V, n, 4)
        a = _dev(alphas, device=self.dev)
        per_view = a.dim() == 2
        a = a.reshape(V, n) if per_view else a.reshape(n)
        c = _dev(colors, device=self.dev)
        c = (c.expand(V, n, 3) if c.dim() == 3 else c.reshape(1, n, 3).expand(V, n, 3)).contiguous()
        tile, n_ty, n_tx = tile_grid(width, height, self.cfg.tile_size)
        idx = _dev(tile_indices, torch.int32, self.dev)
        cnt = _dev(tile_counts, torch.int32, self.dev)
        if tuple(idx.shape) != (V, n_ty, n_tx, self.cap) or tuple(cnt.shape) != (V, n_ty, n_tx):
            raise ValueError(f"tile_indices / tile_counts: expected {(V, n_ty, n_tx, self.cap)} and {(V, n_ty, n_tx)}, "
                             f"got {tuple(idx.shape)} and {tuple(cnt.shape)}")
        shape = (V, int(height), int(width), 3) if image_layout else (V, n_ty, n_tx, tile, tile, 3)
        out = torch.empty(shape, dtype=torch.float64, device=self.dev)
        p = lambda x: x.data_ptr() if n else None   # noqa: E731
        self._stream()
        self._chk(self.lib.gcs_render_tiles(self.h, V, n, int(width), int(height), p(m), p(S), p(a), int(per_view), p(c),
                                            idx.data_ptr(), cnt.data_ptr(), int(bool(image_layout)), out.data_ptr()),
                  "gcs_render_tiles")
        return out

    def render_view(self, positions, covariances, directions, kappas, colors, valid_mask, P_pix, offsets, view_dirs,
                    width: int, height: int, fbm_modulate_scale: float = 0.0, fbm_seed: int = 0,
                    want_splats: bool = False) -> RenderResult:
        """gcs_render_view: prepare, bin and render queued in one call."""
        torch = _torch()
        n, rows = self._rows(positions, covariances, directions, kappas, colors, valid_mask, None)
        V = int(np.asarray(P_pix).reshape(-1, 6).shape[0])
        i, keep = _prepare_inputs(n, V, rows, P_pix, offsets, view_dirs, fbm_modulate_scale, fbm_seed,
                                  lambda x: x.data_ptr())
        t, o = self._splats(V, n) if want_splats else (None, None)
        idx, cnt = self._tile_outputs(V, width, height)
        img = torch.empty((V, int(height), int(width), 3), dtype=torch.float64, device=self.dev)
        self._stream()
        self._chk(self.lib.gcs_render_view(self.h, C.byref(i), int(width), int(height),
                                           C.byref(o) if o is not None else None, idx.data_ptr(), cnt.data_ptr(),
                                           img.data_ptr()), "gcs_render_view")
        return RenderResult(images=img, tile_indices=idx, tile_counts=cnt, splats=t)


_renderers = OrderedDict()
MAX_CACHED_RENDERERS = 8


def renderer_for(cfg: SplatRenderingConfig = SplatRenderingConfig(), device: int = 0) -> Renderer:
    """The cached context of (cfg, device).  At most MAX_CACHED_RENDERERS are kept; the least recently used
    one is closed (its stream and workspace released) when another is needed, so a sweep over parameters
    does not pile contexts up.  A Renderer of one's own is not subject to this."""
    key = (cfg, int(device))
    r = _renderers.get(key)
    if r is None:
        while len(_renderers) >= MAX_CACHED_RENDERERS:
            _renderers.popitem(last=False)[1].close()
        r = _renderers[key] = Renderer(cfg, device)
    _renderers.move_to_end(key)
    return r


def _device_index(x) -> int:
    torch = _torch()
    if isinstance(x, torch.Tensor) and x.is_cuda:
        return x.device.index or 0
    return 0


def splat_indices_for_tiles(means, Sigmas_inv, width: int, height: int, tile_size: int = 32,
                            max_splats_per_tile: int = 64, eps: float = 1e-12):
    """splat_indices_for_tile for every tile of every view: means (V, N, 2) pixels, Sigmas_inv (V, N, 2, 2).
    Returns indices (V, Ty, Tx, max_splats_per_tile) int32 padded with -1 and counts (V, Ty, Tx) int32;
    tile (ty, tx) has origin (oy, ox) = (ty, tx) * tile_size."""
    cfg = SplatRenderingConfig(tile_size=int(tile_size), max_splats_per_tile=int(max_splats_per_tile), eps=float(eps))
    return renderer_for(cfg, _device_index(means)).bin_tiles(means, Sigmas_inv, width, height)


def render_tiles_ewa(means, Sigmas_inv, alphas, colors, tile_indices, tile_counts, width: int, height: int,
                     tile_size: int = 32, log_clip: float = 25.0, means_world_xy=None, fbm_octaves: int = 5,
                     fbm_gain: float = 0.5, fbm_seed: int = 0, fbm_modulate_scale: float = 0.0):
    """render_tile_ewa for every tile of every view: (V, Ty, Tx, tile, tile, 3).  alphas (N,) or (V, N), colors
    (N, 3) or (V, N, 3); with means_world_xy (N, 2) and fbm_modulate_scale > 0 the colours carry the fBm
    factor, as render_tile_ewa applies it."""
    cap = int(tile_indices.shape[-1])
    cfg = SplatRenderingConfig(tile_size=int(tile_size), max_splats_per_tile=cap, ewa_log_clip=float(log_clip))
    r = renderer_for(cfg, _device_index(means))
    c = _dev(colors, device=r.dev)
    if fbm_modulate_scale > 0.0 and means_world_xy is not None:
        fb = fbm_at_splat_positions(_dev(means_world_xy, device=r.dev), fbm_octaves, fbm_gain, fbm_seed)
        c = c * ((1.0 - fbm_modulate_scale) + fbm_modulate_scale * fb)[:, None]
    return r.render_tiles(means, Sigmas_inv, alphas, c, tile_indices, tile_counts, width, height)


def render_map_view(view, tile_ids=None, *, bev: BEVPushforwardConfig = BEVPushforwardConfig(),
                    cfg: SplatRenderingConfig = SplatRenderingConfig(), width: int, height: int,
                    pixels_per_metre: float, centre_xy, fbm_modulate_scale: float = 0.0, fbm_seed: int = 0,
                    m_tile_view: Optional[int] = None, want_splats: bool = False) -> RenderResult:
    """The map as the BEV sweep sees it: view k, angle phi_k, maps a row to pixels by
    mu_px = s P(phi_k) p + b with b = (W/2, H/2) - s P(phi_k) (cx, cy, 0), Sigma_px = s^2 P Sigma P^T; its
    opacity comes from log det Sigma_3D, its colour is clip(view.colors * one-lobe vMF shading against
    (0, sin phi_k, -cos phi_k), 0, 1); fBm enters as render_tile_ewa applies it.  Rows with valid_mask
    false are never listed; indices count the view's rows.  `view`: an AtlasMapView, or an AtlasMap with
    tile_ids (the view is extracted with m_tile_view entries per tile, default the map's m_tile)."""
    if tile_ids is not None:
        from .primitive_map import extract_atlas_map_view
        view = extract_atlas_map_view(view, list(tile_ids), int(m_tile_view or view.m_tile))
    for name in ("covariances", "colors"):
        if getattr(view, name, None) is None:
            raise ValueError(f"render_map_view: the view has no {name}")
    P_pix, offsets, view_dirs = view_geometry(bev, width, height, pixels_per_metre, centre_xy)
    r = renderer_for(cfg, _device_index(view.positions))
    return r.render_view(view.positions, view.covariances, view.directions, view.kappas, view.colors, view.valid_mask,
                         P_pix, offsets, view_dirs, width, height, fbm_modulate_scale, fbm_seed, want_splats)
