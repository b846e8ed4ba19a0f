// Map rendering on the GPU: the reference's output side (backend/rendering.py, common/bev_pushforward.py)
// over an AtlasMapView's rows.  Three kernels, each reachable on its own:
//   k_rn_prepare  one thread per row, looping over the views: pushforward to pixels, adjugate inverse, radius, opacity,
//                 shaded colour, fBm (once per row)                              (gcs_render_math.h)
//   k_rn_bin      one workgroup per (view, tile): streams (mean, radius), keeps the cap smallest
//                 (dist^2, row) pairs exactly -- a threshold filter in front of LDS bitonic sorts
//   k_rn_render   one workgroup per (view, tile): the tile's records staged through LDS 64 at a time,
//                 every thread blends its pixels over the list in list order, in f64
// No float atomics anywhere; the only atomic is the LDS append counter of k_rn_bin, whose order cannot
// reach the result because the sort key (dist^2 bits, row) is unique per row.

#include <hip/hip_runtime.h>

#include <limits.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>

#include "gcs_render_math.h"
#include "gcslam_hip.h"

#pragma clang fp contract(off)

namespace gcs {
namespace {

constexpr int kRnThreads = 256;
constexpr int kRnSort = 2048;                 // LDS sort width: best list (<= 1024) + appended candidates
constexpr int kRnChunkRows = 4 * kRnThreads;  // rows streamed between two looks at the fill
constexpr int kRnRec = 10;                    // mx my s00 s01 s10 s11 alpha r g b
constexpr int kRnStage = 64;                  // records in LDS at once
constexpr int kRnMaxRows = 1 << 28;           // rows per call: the kernels' int row arithmetic stays far from 2^31
static_assert(GCS_RENDER_MAX_CAP + kRnChunkRows <= kRnSort, "a trimmed list plus one chunk fits the sort buffer");

struct RnViews {
  double P[GCS_RENDER_MAX_VIEWS][6], off[GCS_RENDER_MAX_VIEWS][2], vn[GCS_RENDER_MAX_VIEWS][3];
  int n;
};

struct RnRows {
  const double *pos, *cov, *dir, *kappa, *col, *intensity;
  const uint8_t* valid;
  int n;
};

// One row, every view (the body of k_rn_prepare and of gcs_render_prepare_host).
GCS_HD void rn_prepare_row(int i, const RnRows& in, const RnViews& vw, const RnParams& a, const gcs_render_splats& o) {
  const size_t N = (size_t)in.n;
  const double* p = in.pos + 3 * (size_t)i;
  const double* S = in.cov + 9 * (size_t)i;
  bool ok = !in.valid || in.valid[i] != 0;
  // a position that is not finite has no pixel in any view: the whole row is dropped, fBm on or off
  ok = ok && isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]);
  // with fBm on, the lattice index of x * 2^octave (octave < 16) has to fit an int64
  if (a.fbm_scale > 0.0) ok = ok && fabs(p[0]) < 0x1p46 && fabs(p[1]) < 0x1p46;
  // a NaN among the shading's inputs reaches every view's colour (np.clip hands it on): the whole row is dropped
  if (ok) {
    const double* d = in.dir + 3 * (size_t)i;
    const double* c = in.col + 3 * (size_t)i;
    const double k = in.kappa[i], t = in.intensity && a.int_scale > 0.0 ? in.intensity[i] : 0.0;
    ok = !(d[0] != d[0] || d[1] != d[1] || d[2] != d[2] || c[0] != c[0] || c[1] != c[1] || c[2] != c[2] || k != k || t != t);
  }
  double alpha = 0.0, fb = 0.0, mod = 1.0;
  if (ok) {
    alpha = rn_opacity(rn_logdet3(S), a.gamma, a.logdet0, a.alpha_min);
    ok = isfinite(alpha);
  }
  if (ok && a.fbm_scale > 0.0) {
    fb = rn_fbm(p[0], p[1], a.fbm_octaves, a.fbm_gain, a.fbm_seed);
    mod = (1.0 - a.fbm_scale) + a.fbm_scale * fb;
  }
  bool kept = false;   // by some view
  for (int v = 0; v < vw.n; ++v) {
    const size_t k = (size_t)v * N + (size_t)i;
    double mu2[2] = {0.0, 0.0}, Si[4] = {0.0, 0.0, 0.0, 0.0}, r = -INFINITY, c[3] = {0.0, 0.0, 0.0};
    if (ok && rn_push_row(p, S, vw.P[v], vw.off[v], a.eps, mu2, Si, &r)) {
      const double s = rn_shade_one_lobe(vw.vn[v], in.dir + 3 * (size_t)i, in.kappa[i], in.intensity != nullptr,
                                         in.intensity ? in.intensity[i] : 0.0, a);
      bool has_nan = false;   // fmax / fmin return their other argument for a NaN: np.clip would hand it on
      for (int j = 0; j < 3; ++j) {
        const double raw = in.col[3 * (size_t)i + j] * s;
        has_nan = has_nan || raw != raw;
        c[j] = fmin(fmax(raw, 0.0), 1.0) * mod;
      }
      if (has_nan || !(isfinite(c[0]) && isfinite(c[1]) && isfinite(c[2]))) {
        r = -INFINITY;
        mu2[0] = mu2[1] = Si[0] = Si[1] = Si[2] = Si[3] = c[0] = c[1] = c[2] = 0.0;
      } else {
        kept = true;
      }
    }
    o.means[2 * k] = mu2[0]; o.means[2 * k + 1] = mu2[1];
    for (int j = 0; j < 4; ++j) o.Sigmas_inv[4 * k + j] = Si[j];
    o.radii[k] = r;
    for (int j = 0; j < 3; ++j) o.colors[3 * k + j] = c[j];
  }
  // a row that no view keeps is an invalid row's record throughout; one that some views drop keeps its own
  o.alphas[i] = kept ? alpha : 0.0;
  if (o.fbm) o.fbm[i] = kept ? fb : 0.0;
}

__global__ __launch_bounds__(kRnThreads) void k_rn_prepare(RnRows in, RnViews vw, RnParams a, gcs_render_splats o) {
  const int i = blockIdx.x * kRnThreads + threadIdx.x;
  if (i < in.n) rn_prepare_row(i, in, vw, a, o);
}

// radius of every (view, row) from a caller's Sigma^-1 (gcs_render_bin_tiles without radii)
__global__ __launch_bounds__(kRnThreads) void k_rn_radius(const double* __restrict__ Sinv, size_t n, double eps,
                                                          double* __restrict__ r) {
  const size_t k = (size_t)blockIdx.x * kRnThreads + threadIdx.x;
  if (k >= n) return;
  const double rad = rn_radius(Sinv[4 * k], Sinv[4 * k + 2], Sinv[4 * k + 3], eps);
  r[k] = isfinite(rad) ? rad : -INFINITY;
}

__device__ __forceinline__ bool rn_key_less(unsigned long long da, int ra, unsigned long long db, int rb) {
  return da < db || (da == db && ra < rb);
}

// Sorts kd/kr[0, P) ascending by (kd, kr); P a power of two <= kRnSort.  Ends on a barrier.
__device__ void rn_bitonic(unsigned long long* kd, int* kr, int P) {
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < (P >> 1); t += kRnThreads) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
        const unsigned long long di = kd[i], dl = kd[l];
        const int ri = kr[i], rl = kr[l];
        const bool up = (i & k) == 0;
        if (rn_key_less(dl, rl, di, ri) == up) {
          kd[i] = dl; kr[i] = rl;
          kd[l] = di; kr[l] = ri;
        }
      }
      __syncthreads();
    }
}

// grid (n_tx, n_ty, n_views).  splat_indices_for_tile (rendering.py:252-289) for every tile: dist^2 >= 0, so
// its bit pattern orders as the value does; ties fall to the row, which is what Python's stable sort of
// the row-ordered list gives.
__global__ __launch_bounds__(kRnThreads) void k_rn_bin(const double* __restrict__ means, const double* __restrict__ radii,
                                                       int N, int tile, int cap, int32_t* __restrict__ idx_out,
                                                       int32_t* __restrict__ cnt_out) {
  __shared__ unsigned long long kd[kRnSort];
  __shared__ int kr[kRnSort];
  __shared__ int s_n;
  const int tid = threadIdx.x;
  const int tx = blockIdx.x, ty = blockIdx.y, v = blockIdx.z;
  const double ox = (double)(tx * tile), oy = (double)(ty * tile);
  const double cx = ox + 0.5 * (double)tile, cy = oy + 0.5 * (double)tile;
  const double x_max = ox + (double)tile, y_max = oy + (double)tile;
  const double* m = means + 2 * (size_t)v * (size_t)N;
  const double* rr = radii + (size_t)v * (size_t)N;
  if (tid == 0) s_n = 0;
  unsigned long long thr_d = ~0ull;   // the cap-th best so far; nothing at or beyond it can be kept
  int thr_r = INT_MAX;
  __syncthreads();
  for (int base = 0; base < N; base += kRnChunkRows) {
    int n = s_n;
    __syncthreads();   // everyone has read the fill before anyone appends
    if (n > kRnSort - kRnChunkRows) {
      int P = 2;
      while (P < n) P <<= 1;
      for (int t = n + tid; t < P; t += kRnThreads) { kd[t] = ~0ull; kr[t] = INT_MAX; }
      __syncthreads();
      rn_bitonic(kd, kr, P);
      n = min(n, cap);
      if (n == cap) { thr_d = kd[cap - 1]; thr_r = kr[cap - 1]; }
      __syncthreads();   // thresholds read before the tail is overwritten
      if (tid == 0) s_n = n;
      __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = base + k * kRnThreads + tid;
      if (i < N) {
        const double mx = m[2 * (size_t)i], my = m[2 * (size_t)i + 1], r = rr[i];
        if (!(mx + r < ox || mx - r > x_max || my + r < oy || my - r > y_max)) {
          const double dx = mx - cx, dy = my - cy;
          const double d = dx * dx + dy * dy;
          const unsigned long long bits = (unsigned long long)__double_as_longlong(d);
          // a NaN distance (a caller's non-finite mean) is dropped: it has no place in an order
          if (d == d && rn_key_less(bits, i, thr_d, thr_r)) {
            const int pos = atomicAdd(&s_n, 1);   // < kRnSort: the fill was <= kRnSort - kRnChunkRows
            kd[pos] = bits;
            kr[pos] = i;
          }
        }
      }
    }
    __syncthreads();
  }
  int n = s_n;
  __syncthreads();
  if (n > 1) {
    int P = 2;
    while (P < n) P <<= 1;
    for (int t = n + tid; t < P; t += kRnThreads) { kd[t] = ~0ull; kr[t] = INT_MAX; }
    __syncthreads();
    rn_bitonic(kd, kr, P);
  }
  n = min(n, cap);
  const size_t tile_id = ((size_t)v * gridDim.y + ty) * gridDim.x + tx;
  for (int t = tid; t < cap; t += kRnThreads) idx_out[tile_id * (size_t)cap + t] = t < n ? kr[t] : -1;
  if (tid == 0) cnt_out[tile_id] = n;
}

// grid (n_tx, n_ty, n_views).  render_tile_ewa (rendering.py:297-355) for every tile; thread t owns
// pixels t, t + 256, ... of the tile's row-major tile x tile block.
__global__ __launch_bounds__(kRnThreads) void k_rn_render(const double* __restrict__ means, const double* __restrict__ Sinv,
                                                          const double* __restrict__ alphas, int alphas_per_view,
                                                          const double* __restrict__ colors,
                                                          const int32_t* __restrict__ idx, const int32_t* __restrict__ cnt,
                                                          int N, int cap, int tile, int W, int H, double log_clip,
                                                          int image_layout, double* __restrict__ out) {
  __shared__ double rec[kRnStage][kRnRec];
  const int tid = threadIdx.x;
  const int tx = blockIdx.x, ty = blockIdx.y, v = blockIdx.z;
  const size_t tile_id = ((size_t)v * gridDim.y + ty) * gridDim.x + tx;
  const size_t vN = (size_t)v * (size_t)N;
  const int n = min(max(cnt[tile_id], 0), cap);
  const int npix = tile * tile;
  const int ox = tx * tile, oy = ty * tile;
  double acc[4][3], ws[4], px[4], py[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int p = tid + k * kRnThreads;
    acc[k][0] = acc[k][1] = acc[k][2] = ws[k] = 0.0;
    px[k] = (double)(ox + p % tile) + 0.5;
    py[k] = (double)(oy + p / tile) + 0.5;
  }
  for (int base = 0; base < n; base += kRnStage) {
    const int m = min(kRnStage, n - base);
    __syncthreads();   // the previous stage has been consumed
    if (tid < m) {
      const int id = idx[tile_id * (size_t)cap + base + tid];
      double* q = rec[tid];
      if (id >= 0 && id < N) {
        const size_t k = vN + (size_t)id;
        q[0] = means[2 * k]; q[1] = means[2 * k + 1];
        q[2] = Sinv[4 * k]; q[3] = Sinv[4 * k + 1]; q[4] = Sinv[4 * k + 2]; q[5] = Sinv[4 * k + 3];
        q[6] = alphas[alphas_per_view ? k : (size_t)id];
        q[7] = colors[3 * k]; q[8] = colors[3 * k + 1]; q[9] = colors[3 * k + 2];
      } else {
        for (int j = 0; j < kRnRec; ++j) q[j] = 0.0;   // alpha 0: weight 0
      }
    }
    __syncthreads();
    for (int i = 0; i < m; ++i) {
      const double mx = rec[i][0], my = rec[i][1], s00 = rec[i][2], s01 = rec[i][3], s10 = rec[i][4], s11 = rec[i][5];
      const double al = rec[i][6], c0 = rec[i][7], c1 = rec[i][8], c2 = rec[i][9];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (tid + k * kRnThreads < npix) {
          const double d0 = px[k] - mx, d1 = py[k] - my;
          const double q = (d0 * s00 + d1 * s10) * d0 + (d0 * s01 + d1 * s11) * d1;
          const double e = fmin(fmax(-0.5 * fmax(q, 0.0), -log_clip), 0.0);
          const double w = al * exp(e);
          ws[k] += w;
          acc[k][0] += w * c0; acc[k][1] += w * c1; acc[k][2] += w * c2;
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int p = tid + k * kRnThreads;
    if (p >= npix) continue;
    const double total = ws[k] + 1e-12;
    double c[3] = {acc[k][0], acc[k][1], acc[k][2]};
    if (total > 1e-12)
      for (int j = 0; j < 3; ++j) c[j] /= total;
    for (int j = 0; j < 3; ++j) c[j] = fmin(fmax(c[j], 0.0), 1.0);
    size_t o;
    if (image_layout) {
      const int x = ox + p % tile, y = oy + p / tile;
      if (x >= W || y >= H) continue;
      o = (((size_t)v * H + y) * (size_t)W + x) * 3;
    } else {
      o = (tile_id * (size_t)npix + p) * 3;
    }
    out[o] = c[0]; out[o + 1] = c[1]; out[o + 2] = c[2];
  }
}

int rn_tile(const gcs_render_config& c) { return std::min(std::max(c.tile_size, 1), 32); }

RnParams rn_params(const gcs_render_config& c, const gcs_render_prepare_inputs& in) {
  RnParams a{};
  a.gamma = c.opacity_gamma; a.logdet0 = c.logdet0; a.alpha_min = c.alpha_min; a.eps = c.eps;
  a.int_scale = c.vmf_intensity_scale; a.int_max = c.vmf_intensity_max; a.kappa_max = c.vmf_kappa_max;
  a.fbm_gain = c.fbm_gain; a.fbm_scale = in.fbm_modulate_scale; a.fbm_octaves = c.fbm_octaves;
  a.fbm_seed = in.fbm_seed;
  return a;
}

// rendering.py:135-136: v / (|v| + eps), eps the shading's own default
void rn_views(const gcs_render_prepare_inputs& in, RnViews* vw) {
  vw->n = in.n_views;
  for (int v = 0; v < in.n_views; ++v) {
    for (int j = 0; j < 6; ++j) vw->P[v][j] = in.P_pix[6 * v + j];
    for (int j = 0; j < 2; ++j) vw->off[v][j] = in.offsets[2 * v + j];
    const double* d = in.view_dirs + 3 * v;
    const double nrm = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) + kRnNormEps;
    for (int j = 0; j < 3; ++j) vw->vn[v][j] = d[j] / nrm;
  }
}

const char* rn_check_config(const gcs_render_config* c) {
  if (!c) return "null config";
  if (c->max_splats_per_tile < 1 || c->max_splats_per_tile > GCS_RENDER_MAX_CAP)
    return "max_splats_per_tile outside [1, GCS_RENDER_MAX_CAP]";
  if (c->fbm_octaves < 0 || c->fbm_octaves > 16) return "fbm_octaves outside [0, 16]";
  if (!(c->eps > 0.0) || !(c->ewa_log_clip >= 0.0)) return "eps must be > 0 and ewa_log_clip >= 0";
  return nullptr;
}

const char* rn_check_prepare(const gcs_render_prepare_inputs* in, const gcs_render_splats* o) {
  if (!in) return "null inputs";
  if (in->n_rows < 0 || in->n_rows > kRnMaxRows || in->n_views < 1 || in->n_views > GCS_RENDER_MAX_VIEWS)
    return "n_rows outside [0, 2^28] or n_views outside [1, GCS_RENDER_MAX_VIEWS]";
  if (!in->P_pix || !in->offsets || !in->view_dirs) return "null per-view array";
  if (in->n_rows > 0 && (!in->positions || !in->covariances || !in->directions || !in->kappas || !in->colors))
    return "null row array";
  if (o && in->n_rows > 0 && (!o->means || !o->Sigmas_inv || !o->radii || !o->alphas || !o->colors))
    return "null record array";
  return nullptr;
}

}  // namespace
}  // namespace gcs

using namespace gcs;

struct gcs_render_ctx {
  gcs_render_config cfg{};
  std::string err;
  int device = 0;
  hipStream_t own = nullptr, stream = nullptr;
  double* d_ws = nullptr;     // the record of gcs_render_view / the radii of gcs_render_bin_tiles
  size_t ws_doubles = 0;
};

namespace {
int rn_fail(gcs_render_ctx* c, int code, const std::string& m) {
  if (c) c->err = m;
  return code;
}
#define RNCHK(ctx, expr)                                                                          \
  do {                                                                                            \
    hipError_t _e = (expr);                                                                       \
    if (_e != hipSuccess) return rn_fail((ctx), GCS_ERR_HIP, std::string(#expr ": ") + hipGetErrorString(_e)); \
  } while (0)

// grows the workspace (the stream is drained first: a queued kernel may still read the old one)
int rn_workspace(gcs_render_ctx* c, size_t doubles) {
  if (doubles <= c->ws_doubles) return GCS_OK;
  RNCHK(c, hipStreamSynchronize(c->stream));
  if (c->d_ws) (void)hipFree(c->d_ws);
  c->d_ws = nullptr;
  c->ws_doubles = 0;
  RNCHK(c, hipMalloc(&c->d_ws, doubles * sizeof(double)));
  c->ws_doubles = doubles;
  return GCS_OK;
}

int rn_check_image(gcs_render_ctx* c, int n_views, int n_rows, int width, int height) {
  if (n_views < 1 || n_views > GCS_RENDER_MAX_VIEWS || n_rows < 0 || n_rows > kRnMaxRows || width < 1 || height < 1 ||
      width > 16384 || height > 16384)
    return rn_fail(c, GCS_ERR_ARG,
                   "n_views outside [1, GCS_RENDER_MAX_VIEWS], n_rows outside [0, 2^28] or image size outside [1, 16384]");
  return GCS_OK;
}

void rn_queue_prepare(gcs_render_ctx* c, const gcs_render_prepare_inputs& in, const gcs_render_splats& o) {
  if (in.n_rows == 0) return;
  RnViews vw;
  rn_views(in, &vw);
  RnRows rows{in.positions, in.covariances, in.directions, in.kappas, in.colors, in.intensity, in.valid_mask, in.n_rows};
  hipLaunchKernelGGL(k_rn_prepare, dim3((in.n_rows + kRnThreads - 1) / kRnThreads), dim3(kRnThreads), 0, c->stream, rows,
                     vw, rn_params(c->cfg, in), o);
}

void rn_queue_bin(gcs_render_ctx* c, int V, int N, int W, int H, const double* means, const double* radii,
                  int32_t* indices, int32_t* counts) {
  const int tile = rn_tile(c->cfg);
  hipLaunchKernelGGL(k_rn_bin, dim3((W + tile - 1) / tile, (H + tile - 1) / tile, V), dim3(kRnThreads), 0, c->stream, means,
                     radii, N, tile, c->cfg.max_splats_per_tile, indices, counts);
}

void rn_queue_render(gcs_render_ctx* c, int V, int N, int W, int H, const double* means, const double* Sinv,
                     const double* alphas, int per_view, const double* colors, const int32_t* indices,
                     const int32_t* counts, int image_layout, double* out) {
  const int tile = rn_tile(c->cfg);
  hipLaunchKernelGGL(k_rn_render, dim3((W + tile - 1) / tile, (H + tile - 1) / tile, V), dim3(kRnThreads), 0, c->stream,
                     means, Sinv, alphas, per_view, colors, indices, counts, N, c->cfg.max_splats_per_tile, tile, W, H,
                     c->cfg.ewa_log_clip, image_layout, out);
}
}  // namespace

extern "C" {

int gcs_render_config_defaults(gcs_render_config* c) {
  if (!c) return GCS_ERR_ARG;
  memset(c, 0, sizeof(*c));
  c->tile_size = 32;               // rendering.py:32-44
  c->max_splats_per_tile = 64;
  c->fbm_octaves = 5;
  c->fbm_gain = 0.5;
  c->opacity_gamma = 1.0;
  c->logdet0 = 0.0;
  c->eps = 1e-12;
  c->ewa_log_clip = 25.0;
  c->alpha_min = 0.02;
  c->vmf_intensity_scale = 0.5;
  c->vmf_intensity_max = 255.0;
  c->vmf_kappa_max = 100.0;
  c->device = 0;
  return GCS_OK;
}

const char* gcs_render_last_error(const gcs_render_ctx* c) { return c ? c->err.c_str() : "null render context"; }

int gcs_render_ctx_destroy(gcs_render_ctx* c) {
  if (!c) return GCS_OK;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->d_ws) (void)hipFree(c->d_ws);
  if (c->own) (void)hipStreamDestroy(c->own);
  delete c;
  return GCS_OK;
}

int gcs_render_ctx_create(const gcs_render_config* cfg, gcs_render_ctx** out) {
  if (!cfg || !out) return GCS_ERR_ARG;
  *out = nullptr;
  if (rn_check_config(cfg)) return GCS_ERR_ARG;
  auto* c = new gcs_render_ctx();
  c->cfg = *cfg;
  c->device = cfg->device;
  if (hipSetDevice(cfg->device) != hipSuccess ||
      hipStreamCreateWithFlags(&c->own, hipStreamNonBlocking) != hipSuccess) {
    gcs_render_ctx_destroy(c);
    return GCS_ERR_HIP;
  }
  c->stream = c->own;
  *out = c;
  return GCS_OK;
}

int gcs_render_ctx_set_stream(gcs_render_ctx* c, void* stream) {
  if (!c) return GCS_ERR_ARG;
  hipStream_t ns = stream ? (hipStream_t)stream : c->own;
  if (ns == c->stream) return GCS_OK;
  RNCHK(c, hipSetDevice(c->device));
  RNCHK(c, hipStreamSynchronize(c->stream));  // work queued on the old stream completes first
  c->stream = ns;
  return GCS_OK;
}

int gcs_render_prepare_host(const gcs_render_config* cfg, const gcs_render_prepare_inputs* in, gcs_render_splats* out) {
  if (rn_check_config(cfg) || !out || rn_check_prepare(in, out)) return GCS_ERR_ARG;
  RnViews vw;
  rn_views(*in, &vw);
  const RnParams a = rn_params(*cfg, *in);
  RnRows rows{in->positions, in->covariances, in->directions, in->kappas, in->colors, in->intensity, in->valid_mask,
              in->n_rows};
  for (int i = 0; i < in->n_rows; ++i) rn_prepare_row(i, rows, vw, a, *out);
  return GCS_OK;
}

int gcs_render_prepare(gcs_render_ctx* c, const gcs_render_prepare_inputs* in, gcs_render_splats* out) {
  if (!c || !out) return GCS_ERR_ARG;
  if (const char* m = rn_check_prepare(in, out)) return rn_fail(c, GCS_ERR_ARG, m);
  RNCHK(c, hipSetDevice(c->device));
  rn_queue_prepare(c, *in, *out);
  RNCHK(c, hipGetLastError());
  RNCHK(c, hipStreamSynchronize(c->stream));
  return GCS_OK;
}

int gcs_render_bin_tiles(gcs_render_ctx* c, int32_t V, int32_t N, int32_t W, int32_t H, const double* means,
                         const double* radii, const double* Sinv, int32_t* indices, int32_t* counts) {
  if (!c) return GCS_ERR_ARG;
  if (int rc = rn_check_image(c, V, N, W, H)) return rc;
  if (!indices || !counts || (N > 0 && (!means || (!radii && !Sinv))))
    return rn_fail(c, GCS_ERR_ARG, "null array");
  RNCHK(c, hipSetDevice(c->device));
  if (N > 0 && !radii) {
    const size_t n = (size_t)V * (size_t)N;
    if (int rc = rn_workspace(c, n)) return rc;
    hipLaunchKernelGGL(k_rn_radius, dim3((unsigned)((n + kRnThreads - 1) / kRnThreads)), dim3(kRnThreads), 0, c->stream,
                       Sinv, n, c->cfg.eps, c->d_ws);
    radii = c->d_ws;
  }
  rn_queue_bin(c, V, N, W, H, means, radii, indices, counts);
  RNCHK(c, hipGetLastError());
  RNCHK(c, hipStreamSynchronize(c->stream));
  return GCS_OK;
}

int gcs_render_tiles(gcs_render_ctx* c, int32_t V, int32_t N, int32_t W, int32_t H, const double* means,
                     const double* Sinv, const double* alphas, int32_t per_view, const double* colors,
                     const int32_t* indices, const int32_t* counts, int32_t image_layout, double* out) {
  if (!c) return GCS_ERR_ARG;
  if (int rc = rn_check_image(c, V, N, W, H)) return rc;
  if (!indices || !counts || !out || (N > 0 && (!means || !Sinv || !alphas || !colors)))
    return rn_fail(c, GCS_ERR_ARG, "null array");
  RNCHK(c, hipSetDevice(c->device));
  rn_queue_render(c, V, N, W, H, means, Sinv, alphas, per_view != 0, colors, indices, counts, image_layout != 0, out);
  RNCHK(c, hipGetLastError());
  RNCHK(c, hipStreamSynchronize(c->stream));
  return GCS_OK;
}

int gcs_render_view(gcs_render_ctx* c, const gcs_render_prepare_inputs* in, int32_t W, int32_t H,
                    gcs_render_splats* splats, int32_t* indices, int32_t* counts, double* images) {
  if (!c) return GCS_ERR_ARG;
  if (const char* m = rn_check_prepare(in, nullptr)) return rn_fail(c, GCS_ERR_ARG, m);
  if (int rc = rn_check_image(c, in->n_views, in->n_rows, W, H)) return rc;
  if (!indices || !counts || !images) return rn_fail(c, GCS_ERR_ARG, "null output array");
  RNCHK(c, hipSetDevice(c->device));
  const size_t V = (size_t)in->n_views, N = (size_t)in->n_rows;
  gcs_render_splats s{};
  if (splats && splats->means && splats->Sigmas_inv && splats->radii && splats->alphas && splats->colors) {
    s = *splats;
  } else if (N > 0) {
    if (int rc = rn_workspace(c, V * N * 10 + 2 * N)) return rc;
    double* w = c->d_ws;
    s.means = w;                 w += 2 * V * N;
    s.Sigmas_inv = w;            w += 4 * V * N;
    s.radii = w;                 w += V * N;
    s.colors = w;                w += 3 * V * N;
    s.alphas = w;                w += N;
    s.fbm = w;
  }
  rn_queue_prepare(c, *in, s);
  rn_queue_bin(c, (int)V, (int)N, W, H, s.means, s.radii, indices, counts);
  rn_queue_render(c, (int)V, (int)N, W, H, s.means, s.Sigmas_inv, s.alphas, 0, s.colors, indices, counts, 1, images);
  RNCHK(c, hipGetLastError());
  RNCHK(c, hipStreamSynchronize(c->stream));
  return GCS_OK;
}

}  // extern "C"
