// Visual features on the GPU: the per-keypoint numerics of the reference's visual feature node
// (src/visual_feature_node.cpp:493-652, after ORB) from a depth image and a keypoint list to the feature
// arrays gcs_camsplat_inputs reads.  Kernels:
//   k_vf_rank      one thread per keypoint: its place in the (response desc, index asc) order, by counting
//   k_vf_compact   one workgroup: the kept keypoints' indices in input order (a block scan)
//   k_vf_features  one wave64 per output row, four waves per workgroup, one lane per window pixel:
//                  lanes [0, n_sample) hold the depth sample's window (1, 9, 25 or the 7 hex taps), then
//                  lanes [0, (2r + 1)^2) the fit's; the median is picked by rank count over the wave
//                  (ties by lane), the sums are butterflies (x += shfl_xor(x, off), off = 32 .. 1, the same
//                  order every run, no atomics); lane 0 solves the 6 x 6 system and writes the row.
// The first two run only when there are more keypoints than max_features.  The math is gcs_visfeat_math.h,
// which gcs_visual_features_host steps through on the host with 64 lanes in a loop.

#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "gcs_visfeat_math.h"
#include "gcslam_hip.h"

#pragma clang fp contract(off)

namespace gcs {
namespace {

constexpr int kVfWaves = 4;                       // waves (rows) per workgroup
constexpr int kVfThreads = kVfWaves * kVfLanes;
constexpr int kVfSelThreads = 256;
constexpr int kVfScanThreads = 1024;
constexpr int kVfMaxKeypoints = 1 << 16;   // k_vf_rank counts n^2 pairs

__device__ inline double vf_wave_sum(double x) {
  for (int off = kVfLanes / 2; off > 0; off >>= 1) x += __shfl_xor(x, off, kVfLanes);
  return x;
}

// the value of rank `want` among the lanes of `mask` (vf_before's order); every lane gets it
__device__ inline double vf_wave_select(double z, bool ok, unsigned long long mask, int n_lanes, int want, int lane) {
  int rank = 0;
  for (int j = 0; j < n_lanes; ++j) {
    const double zj = __shfl(z, j, kVfLanes);
    if (((mask >> j) & 1ull) && vf_before(zj, j, z, lane)) ++rank;
  }
  const unsigned long long hit = __ballot(ok && rank == want);
  return __shfl(z, hit ? __ffsll((long long)hit) - 1 : 0, kVfLanes);
}

__global__ __launch_bounds__(kVfThreads) void k_vf_features(VfImage im, VfParams p, const float* __restrict__ kp_u,
                                                            const float* __restrict__ kp_v,
                                                            const float* __restrict__ kp_r,
                                                            int n_keypoints, const int32_t* __restrict__ sel,
                                                            int count, int max_features, gcs_visfeat_outputs o) {
  const int lane = threadIdx.x & (kVfLanes - 1);
  const int row = blockIdx.x * kVfWaves + (threadIdx.x >> 6);
  if (row >= max_features) return;   // (uniform over the wave, as every branch around a cross-lane step below)
  if (row >= count) {
    if (lane == 0) vf_zero_row(row, o);
    return;
  }
  VfKeypoint k;
  k.kp_index = sel ? sel[row] : row;
  if ((unsigned)k.kp_index >= (unsigned)n_keypoints) {   // (cannot happen: the selection keeps exactly count indices)
    if (lane == 0) vf_zero_row(row, o);
    return;
  }
  k.u = (double)kp_u[k.kp_index];
  k.v = (double)kp_v[k.kp_index];
  k.response = (double)kp_r[k.kp_index];
  int x, y, dx, dy;
  const bool inside = vf_pixel(k.u, k.v, im, &x, &y);

  // depth sample (:228-348)
  double z = 0.0;
  bool ok = false;
  if (inside && vf_sample_offset(p, lane, &dx, &dy)) ok = vf_depth_at(im, p.depth_scale, x + dx, y + dy, &z);
  const unsigned long long mask = __ballot(ok);
  const int n = __popcll(mask);
  k.n_depth = n;
  k.n_zs = p.mode == GCS_VF_NEAREST ? 0 : n;
  k.z_valid = p.mode == GCS_VF_HEX ? n >= 4 : n >= 1;
  k.z_m = k.z_var = NAN;
  k.q_sum = 0.0;
  if (k.z_valid) {
    k.z_m = vf_wave_select(z, ok, mask, p.n_sample_lanes, n / 2, lane);
    if (p.mode == GCS_VF_HEX) {
      const double mad = vf_wave_select(fabs(z - k.z_m), ok, mask, p.n_sample_lanes, n / 2, lane);
      const double s = 1.4826 * mad;
      k.z_var = s * s;
    } else if (p.mode != GCS_VF_NEAREST && n >= 4) {
      const double mean = vf_wave_sum(ok ? z : 0.0) / (double)n;
      const double d = z - mean;
      k.z_var = vf_wave_sum(ok ? d * d : 0.0) / (double)n;
    }
    const double r = z - k.z_m;
    k.q_sum = vf_wave_sum(ok ? r * r : 0.0);
  }

  // the fit's sums (:409-444)
  k.n_fit = 0;
  if (k.z_valid) {
    double zf = 0.0;
    const bool in_win = vf_fit_offset(p, lane, &dx, &dy);
    const bool okf = in_win && vf_depth_at(im, p.depth_scale, x + dx, y + dy, &zf);
    k.n_fit = __popcll(__ballot(okf));
    if (k.n_fit >= p.quad_min_points) {
      double t[kVfSums];
      vf_fit_terms((double)(x + dx) - k.u, (double)(y + dy) - k.v, zf, t);
      for (int j = 0; j < kVfSums; ++j) k.sums[j] = vf_wave_sum(okf ? t[j] : 0.0);
    }
  }
  if (lane == 0) vf_finish(p, im, k, row, o);
}

__global__ __launch_bounds__(kVfSelThreads) void k_vf_rank(const float* __restrict__ resp, int n, int max_features,
                                                          int32_t* __restrict__ keep) {
  __shared__ float s[kVfSelThreads];
  const int i = blockIdx.x * kVfSelThreads + threadIdx.x;
  const float ri = i < n ? resp[i] : 0.0f;
  int rank = 0;
  for (int base = 0; base < n; base += kVfSelThreads) {
    const int j0 = base + (int)threadIdx.x;
    s[threadIdx.x] = j0 < n ? resp[j0] : 0.0f;
    __syncthreads();
    const int m = min(kVfSelThreads, n - base);
    for (int q = 0; q < m; ++q)
      if (vf_resp_before(s[q], base + q, ri, i)) ++rank;
    __syncthreads();
  }
  if (i < n) keep[i] = rank < max_features ? 1 : 0;
}

__global__ __launch_bounds__(kVfScanThreads) void k_vf_compact(const int32_t* __restrict__ keep, int n, int max_features,
                                                              int32_t* __restrict__ sel) {
  __shared__ int s[kVfScanThreads];
  const int t = threadIdx.x;
  const int per = (n + kVfScanThreads - 1) / kVfScanThreads;
  const int lo = min(n, t * per), hi = min(n, lo + per);
  int c = 0;
  for (int i = lo; i < hi; ++i) c += keep[i];
  s[t] = c;
  __syncthreads();
  for (int off = 1; off < kVfScanThreads; off <<= 1) {   // inclusive scan
    const int add = t >= off ? s[t - off] : 0;
    __syncthreads();
    s[t] += add;
    __syncthreads();
  }
  int pos = s[t] - c;
  for (int i = lo; i < hi; ++i)
    if (keep[i]) {
      if (pos < max_features) sel[pos] = i;
      ++pos;
    }
}

// ---- host build of the same rows

double vf_host_sum(double* x) {   // the wave's butterfly: every lane ends with the same value
  double t[kVfLanes];
  for (int off = kVfLanes / 2; off > 0; off >>= 1) {
    for (int l = 0; l < kVfLanes; ++l) t[l] = x[l] + x[l ^ off];
    memcpy(x, t, sizeof(t));
  }
  return x[0];
}

double vf_host_select(const double* z, const bool* ok, int n_lanes, int want) {
  for (int i = 0; i < n_lanes; ++i) {
    if (!ok[i]) continue;
    int rank = 0;
    for (int j = 0; j < n_lanes; ++j)
      if (ok[j] && vf_before(z[j], j, z[i], i)) ++rank;
    if (rank == want) return z[i];
  }
  return z[0];
}

void vf_host_row(const VfImage& im, const VfParams& p, const gcs_visfeat_inputs& in, int ki, int row,
                 const gcs_visfeat_outputs& o) {
  VfKeypoint k;
  k.kp_index = ki;
  k.u = (double)in.kp_u[ki];
  k.v = (double)in.kp_v[ki];
  k.response = (double)in.kp_response[ki];
  int x, y, dx, dy;
  const bool inside = vf_pixel(k.u, k.v, im, &x, &y);
  double z[kVfLanes], w[kVfLanes];
  bool ok[kVfLanes];
  int n = 0;
  for (int l = 0; l < kVfLanes; ++l) {
    z[l] = 0.0;
    ok[l] = inside && vf_sample_offset(p, l, &dx, &dy) && vf_depth_at(im, p.depth_scale, x + dx, y + dy, &z[l]);
    n += ok[l];
  }
  k.n_depth = n;
  k.n_zs = p.mode == GCS_VF_NEAREST ? 0 : n;
  k.z_valid = p.mode == GCS_VF_HEX ? n >= 4 : n >= 1;
  k.z_m = k.z_var = NAN;
  k.q_sum = 0.0;
  if (k.z_valid) {
    k.z_m = vf_host_select(z, ok, p.n_sample_lanes, n / 2);
    if (p.mode == GCS_VF_HEX) {
      for (int l = 0; l < kVfLanes; ++l) w[l] = fabs(z[l] - k.z_m);
      const double s = 1.4826 * vf_host_select(w, ok, p.n_sample_lanes, n / 2);
      k.z_var = s * s;
    } else if (p.mode != GCS_VF_NEAREST && n >= 4) {
      for (int l = 0; l < kVfLanes; ++l) w[l] = ok[l] ? z[l] : 0.0;
      const double mean = vf_host_sum(w) / (double)n;
      for (int l = 0; l < kVfLanes; ++l) w[l] = ok[l] ? (z[l] - mean) * (z[l] - mean) : 0.0;
      k.z_var = vf_host_sum(w) / (double)n;
    }
    for (int l = 0; l < kVfLanes; ++l) w[l] = ok[l] ? (z[l] - k.z_m) * (z[l] - k.z_m) : 0.0;
    k.q_sum = vf_host_sum(w);
  }
  k.n_fit = 0;
  if (k.z_valid) {
    static thread_local double t[kVfLanes][kVfSums];
    for (int l = 0; l < kVfLanes; ++l) {
      double zf = 0.0;
      ok[l] = vf_fit_offset(p, l, &dx, &dy) && vf_depth_at(im, p.depth_scale, x + dx, y + dy, &zf);
      k.n_fit += ok[l];
      vf_fit_terms((double)(x + dx) - k.u, (double)(y + dy) - k.v, zf, t[l]);
    }
    if (k.n_fit >= p.quad_min_points)
      for (int j = 0; j < kVfSums; ++j) {
        for (int l = 0; l < kVfLanes; ++l) w[l] = ok[l] ? t[l][j] : 0.0;
        k.sums[j] = vf_host_sum(w);
      }
  }
  vf_finish(p, im, k, row, o);
}

const char* vf_check_config(const gcs_visfeat_config* c) {
  if (!c) return "null config";
  if (c->quad_fit_radius > 3) return "quad_fit_radius above 3";
  if (c->hex_radius > 32) return "hex_radius above 32";
  if (c->max_features < 1) return "max_features below 1";
  if (c->max_keypoints < c->max_features || c->max_keypoints > kVfMaxKeypoints)
    return "max_keypoints below max_features or above 65536";
  if (c->depth_sample_mode < GCS_VF_NEAREST || c->depth_sample_mode > GCS_VF_HEX) return "unknown depth_sample_mode";
  if (c->depth_model != GCS_VF_DEPTH_LINEAR && c->depth_model != GCS_VF_DEPTH_QUADRATIC) return "unknown depth_model";
  return nullptr;
}

const char* vf_check_call(const gcs_visfeat_config& c, const gcs_visfeat_inputs* in, const gcs_visfeat_outputs* o) {
  if (!in || !o) return "null inputs or outputs";
  if (!in->depth || in->width < 1 || in->height < 1 || in->width > 65536 || in->height > 65536)
    return "null depth image or image size outside [1, 65536]";
  if (in->depth_format != 0 && in->depth_format != 1) return "depth_format is 0 (float32) or 1 (uint16)";
  const int64_t el = in->depth_format == 1 ? 2 : 4;
  if (in->depth_pitch < el * in->width || in->depth_pitch % el) return "depth_pitch below a row or not a multiple of the value size";
  if (in->rgb && in->rgb_pitch < 3 * (int64_t)in->width) return "rgb_pitch below a row";
  if (!(std::isfinite(in->fx) && std::isfinite(in->fy) && std::isfinite(in->cx) && std::isfinite(in->cy)) ||
      !(in->fx > 0.0) || !(in->fy > 0.0))
    return "intrinsics: finite fx, fy > 0, cx, cy";
  if (in->n_keypoints < 0 || in->n_keypoints > c.max_keypoints) return "n_keypoints outside [0, max_keypoints]";
  if (in->n_keypoints > 0 && (!in->kp_u || !in->kp_v || !in->kp_response)) return "null keypoint array";
  if (!o->u || !o->v || !o->xyz || !o->cov || !o->weight || !o->kappa_app || !o->mu_app || !o->has_mu || !o->color ||
      !o->has_color || !o->depth_Lambda_c || !o->depth_theta_c)
    return "null feature array";
  return nullptr;
}

VfImage vf_image(const gcs_visfeat_inputs& in) {
  VfImage im{};
  im.depth = in.depth; im.rgb = in.rgb;
  im.depth_pitch = in.depth_pitch; im.rgb_pitch = in.rgb_pitch;
  im.depth_format = in.depth_format; im.width = in.width; im.height = in.height;
  return im;
}

VfParams vf_params(const gcs_visfeat_config& c, const gcs_visfeat_inputs& in) {
  VfParams p{};
  p.mode = c.depth_sample_mode; p.model = c.depth_model;
  p.quad_r = std::max(1, c.quad_fit_radius);
  p.quad_min_points = c.quad_fit_min_points;
  const int n_lanes[4] = {1, 9, 25, 7};
  p.n_sample_lanes = n_lanes[p.mode];
  const int r = std::max(1, c.hex_radius);   // :303-312, on the host's libm as the node's
  for (int k = 0; k < 6; ++k) {
    const double ang = static_cast<double>(k) * M_PI / 3.0;
    p.hex_dx[k + 1] = static_cast<int>(std::round(r * std::cos(ang)));
    p.hex_dy[k + 1] = static_cast<int>(std::round(r * std::sin(ang)));
  }
  p.fx = in.fx; p.fy = in.fy; p.cx = in.cx; p.cy = in.cy;
  p.pixel_sigma = c.pixel_sigma; p.depth_sigma0 = c.depth_sigma0; p.depth_sigma_slope = c.depth_sigma_slope;
  p.min_depth_m = c.min_depth_m; p.max_depth_m = c.max_depth_m; p.depth_validity_slope = c.depth_validity_slope;
  p.response_soft_scale = c.response_soft_scale; p.depth_scale = c.depth_scale;
  p.invalid_cov_inflate = c.invalid_cov_inflate; p.quad_fit_lstsq_eps = c.quad_fit_lstsq_eps;
  p.student_t_nu = c.student_t_nu; p.student_t_w_min = c.student_t_w_min;
  p.ma_tau = c.ma_tau; p.ma_delta_inflate = c.ma_delta_inflate;
  p.kappa0 = c.kappa0; p.kappa_alpha = c.kappa_alpha; p.kappa_max = c.kappa_max; p.kappa_min = c.kappa_min;
  return p;
}

}  // namespace
}  // namespace gcs

using namespace gcs;

struct gcs_visfeat_ctx {
  gcs_visfeat_config cfg{};
  std::string err;
  int device = 0;
  hipStream_t stream = nullptr;   // the caller's (gcs_visfeat_ctx_set_stream); null: HIP's default stream
  int32_t *d_keep = nullptr, *d_sel = nullptr;   // max_keypoints flags, max_features kept indices
};

namespace {
int vf_fail(gcs_visfeat_ctx* c, int code, const std::string& m) {
  if (c) c->err = m;
  return code;
}
#define VFCHK(ctx, expr)                                                                          \
  do {                                                                                            \
    hipError_t _e = (expr);                                                                       \
    if (_e != hipSuccess) return vf_fail((ctx), GCS_ERR_HIP, std::string(#expr ": ") + hipGetErrorString(_e)); \
  } while (0)
}  // namespace

extern "C" {

int gcs_visfeat_config_defaults(gcs_visfeat_config* c) {
  if (!c) return GCS_ERR_ARG;
  memset(c, 0, sizeof(*c));
  c->max_features = 512;                     // visual_feature_node.cpp:70-101
  c->depth_sample_mode = GCS_VF_MEDIAN3;
  c->depth_model = GCS_VF_DEPTH_LINEAR;
  c->hex_radius = 2;
  c->quad_fit_radius = 2;
  c->quad_fit_min_points = 6;
  c->pixel_sigma = 1.0;
  c->depth_sigma0 = 0.01;
  c->depth_sigma_slope = 0.01;
  c->min_depth_m = 0.05;
  c->max_depth_m = 80.0;
  c->depth_validity_slope = 5.0;
  c->response_soft_scale = 50.0;
  c->depth_scale = 1.0;
  c->cov_reg_eps = 1e-9;
  c->invalid_cov_inflate = 1e6;
  c->quad_fit_lstsq_eps = 1e-8;
  c->student_t_nu = 3.0;
  c->student_t_w_min = 0.1;
  c->ma_tau = 10.0;
  c->ma_delta_inflate = 1e-4;
  c->kappa0 = 1.0;
  c->kappa_alpha = 10.0;
  c->kappa_max = 100.0;
  c->kappa_min = 0.1;
  c->max_keypoints = 4096;
  c->device = 0;
  return GCS_OK;
}

const char* gcs_visfeat_last_error(const gcs_visfeat_ctx* c) { return c ? c->err.c_str() : "null visfeat context"; }

int gcs_visfeat_ctx_destroy(gcs_visfeat_ctx* c) {
  if (!c) return GCS_OK;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  if (c->d_keep) (void)hipFree(c->d_keep);
  if (c->d_sel) (void)hipFree(c->d_sel);
  delete c;
  return GCS_OK;
}

int gcs_visfeat_ctx_create(const gcs_visfeat_config* cfg, gcs_visfeat_ctx** out) {
  if (!cfg || !out) return GCS_ERR_ARG;
  *out = nullptr;
  if (vf_check_config(cfg)) return GCS_ERR_ARG;
  auto* c = new gcs_visfeat_ctx();
  c->cfg = *cfg;
  c->device = cfg->device;
  if (hipSetDevice(cfg->device) != hipSuccess ||
      hipMalloc(&c->d_keep, sizeof(int32_t) * (size_t)cfg->max_keypoints) != hipSuccess ||
      hipMalloc(&c->d_sel, sizeof(int32_t) * (size_t)cfg->max_features) != hipSuccess) {
    gcs_visfeat_ctx_destroy(c);
    return GCS_ERR_HIP;
  }
  *out = c;
  return GCS_OK;
}

int gcs_visfeat_ctx_set_stream(gcs_visfeat_ctx* c, void* stream) {
  if (!c) return GCS_ERR_ARG;
  hipStream_t ns = (hipStream_t)stream;
  if (ns == c->stream) return GCS_OK;
  VFCHK(c, hipSetDevice(c->device));
  VFCHK(c, hipStreamSynchronize(c->stream));  // the selection scratch is shared: the old stream's work completes first
  c->stream = ns;
  return GCS_OK;
}

int gcs_visual_features_host(const gcs_visfeat_config* cfg, const gcs_visfeat_inputs* in, gcs_visfeat_outputs* out) {
  if (vf_check_config(cfg) || vf_check_call(*cfg, in, out)) return GCS_ERR_ARG;
  const VfImage im = vf_image(*in);
  const VfParams p = vf_params(*cfg, *in);
  const int n = in->n_keypoints, cap = cfg->max_features, count = std::min(n, cap);
  std::vector<int32_t> sel;
  if (n > cap)   // the cap largest responses, ties to the lower index, in input order
    for (int i = 0; i < n; ++i) {
      int rank = 0;
      for (int j = 0; j < n; ++j) rank += vf_resp_before(in->kp_response[j], j, in->kp_response[i], i);
      if (rank < cap) sel.push_back(i);
    }
  for (int r = 0; r < count; ++r) vf_host_row(im, p, *in, sel.empty() ? r : sel[r], r, *out);
  for (int r = count; r < cap; ++r) vf_zero_row(r, *out);
  out->count = count;
  return GCS_OK;
}

int gcs_visual_features(gcs_visfeat_ctx* c, const gcs_visfeat_inputs* in, gcs_visfeat_outputs* out) {
  if (!c) return GCS_ERR_ARG;
  if (const char* m = vf_check_call(c->cfg, in, out)) return vf_fail(c, GCS_ERR_ARG, m);
  VFCHK(c, hipSetDevice(c->device));
  const int n = in->n_keypoints, cap = c->cfg.max_features, count = std::min(n, cap);
  const int32_t* sel = nullptr;
  if (n > cap) {
    hipLaunchKernelGGL(k_vf_rank, dim3((n + kVfSelThreads - 1) / kVfSelThreads), dim3(kVfSelThreads), 0, c->stream,
                       in->kp_response, n, cap, c->d_keep);
    hipLaunchKernelGGL(k_vf_compact, dim3(1), dim3(kVfScanThreads), 0, c->stream, c->d_keep, n, cap, c->d_sel);
    sel = c->d_sel;
  }
  gcs_visfeat_outputs o = *out;
  hipLaunchKernelGGL(k_vf_features, dim3((cap + kVfWaves - 1) / kVfWaves), dim3(kVfThreads), 0, c->stream, vf_image(*in),
                     vf_params(c->cfg, *in), in->kp_u, in->kp_v, in->kp_response, n, sel, count, cap, o);
  VFCHK(c, hipGetLastError());
  out->count = count;
  return GCS_OK;
}

}  // extern "C"
