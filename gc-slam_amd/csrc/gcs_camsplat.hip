// Camera splats on gfx950 -- the camera half of the live primitive path's measurement batch
// (FS/backend/backend_node.py:1865-1925): lidar_depth_evidence and splat_prep_fused
// (FS/frontend/sensors/lidar_camera_depth_fusion.py, splat_prep.py), the node's base-frame conversion
// and the camera slice of FS/backend/structures/measurement_batch.py:165-259.
//
//   k_cs_box       the query pixels' bounding box grown by the radius; clears the call's counters
//   k_cs_count     per point: p_cam = R^T (p - t), z > 0, pixel (u, v) (:80-96, :123); per block the
//                  count of points in front of the camera and of those inside the box; the points are an
//                  n x 3 f64 array or the scan's own records (CsPts: float32 widened exactly, same bits)
//   k_cs_offsets   one workgroup: exclusive scan of the block counts
//   k_cs_compact   the projected table (u, v, x, y, z of the kept points), stable in point order
//   k_cs_feature   one workgroup per feature: candidates within the radius into LDS in point order
//                  (wave ballots, waves in sequence), Route A (:99-164: exact median / MAD by rank
//                  selection, population variance), Route B (:242-386: the nearest points of the pixel
//                  ray by rank, plane fit on one wave, softplus depth, reliabilities), the product of
//                  experts and the splat (splat_prep.py:73-133), base frame, information form
//   k_cs_finish    padding rows; every row zeroed when a feature overflowed max_candidates
// Everything is f64 and fixed-order (no floating-point atomics): two runs are bitwise equal.  The
// file is compiled without floating-point contraction: the projection and the in-radius test are the
// reference's separate multiplies and adds, so the integer decisions (candidate sets) match it.
#include <hip/hip_runtime.h>

#include <limits.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>

#include "gcs_live.h"
#include "gcs_math.h"
#include "gcslam_hip.h"

#pragma clang fp contract(off)

namespace gcs {
namespace {

constexpr int kCsThreads = 256;
constexpr int kCsWaves = kCsThreads / 64;
constexpr int kCsMaxCand = 1024;   // LDS: 4 B index + 8 B depth + 8 B ray distance per candidate = 20 KB
constexpr int kCsMaxFit = 64;      // Route B's fitted points: one lane each
constexpr double kMadScale = 1.4826;   // MAD_NORMAL_SCALE (:21)

struct CsParams {
  double R[9], t[3], fx, fy, cx, cy;
  double w_cam, w_lidar, gamma, r2, base_sigma, var_min, n0, alpha_cnt, beta_mad, gamma_repr;
  double delta, alpha_angle, t_angle, beta_planar, rho0, gamma_res, fit_eps, z_min, sigma_max_sq, alpha_z;
  double pix_var, eps_lift, timestamp, box_margin;
  int min_points, fit_max, max_cand, n_feat;
};

struct CsIn {
  const double *u, *v, *Lc, *thc, *xyz, *cov, *weight, *kappa, *mu, *color;
  const uint8_t *has_mu, *has_color;
};

struct CsOut {
  double *Lambdas, *thetas, *etas, *weights, *timestamps, *colors;
  int32_t *sources, *source_indices;
  uint8_t* valid_mask;
  int32_t* n_pt;
  double *z_med, *mad, *Lambda_A, *theta_A, *Lambda_B, *theta_B, *z_f;
  uint8_t* fused;
};

// counters of one call (device): [0] table entries, [1] points with z > 0, [2] first overflowing feature
constexpr int kCntTab = 0, kCntPos = 1, kCntErr = 2;

// the points: records of `step` bytes with x, y, z at their start -- fmt 0: float32 at bytes 0, 4, 8 (the
// scan's PointCloud2 records, gcs_scan_inputs.xyz_dev), widened exactly; fmt 1: float64 at bytes 0, 8, 16
// (an n x 3 f64 array is fmt 1 with step 24)
struct CsPts {
  const void* base;
  int step, fmt;
};

// p_cam = R^T (p - t) and the pixel of _project_camera (:92-94); true where z > 0
__device__ __forceinline__ bool cs_project(const CsPts& s, int i, const CsParams& a, double* pc, double* u,
                                           double* v) {
  const char* rec = (const char*)s.base + (size_t)i * (size_t)s.step;
  double px, py, pz;
  if (s.fmt == 0) {
    const float* f = (const float*)rec;
    px = (double)f[0]; py = (double)f[1]; pz = (double)f[2];
  } else {
    const double* d = (const double*)rec;
    px = d[0]; py = d[1]; pz = d[2];
  }
  const double dx = px - a.t[0], dy = py - a.t[1], dz = pz - a.t[2];
  pc[0] = a.R[0] * dx + a.R[3] * dy + a.R[6] * dz;
  pc[1] = a.R[1] * dx + a.R[4] * dy + a.R[7] * dz;
  pc[2] = a.R[2] * dx + a.R[5] * dy + a.R[8] * dz;
  const double zz = pc[2] + 1e-12;
  *u = a.fx * (pc[0] / zz) + a.cx;
  *v = a.fy * (pc[1] / zz) + a.cy;
  return pc[2] > 0.0;
}

__device__ __forceinline__ bool cs_in_box(double u, double v, const double* box) {
  return u >= box[0] && u <= box[1] && v >= box[2] && v <= box[3];
}

__global__ __launch_bounds__(kCsThreads) void k_cs_box(const double* __restrict__ u, const double* __restrict__ v,
                                                        int m, double margin, double* __restrict__ box,
                                                        int32_t* __restrict__ cnt) {
  __shared__ double lds[kCsWaves][4];
  double b[4] = {INFINITY, -INFINITY, INFINITY, -INFINITY};   // u min, u max, v min, v max
  for (int i = threadIdx.x; i < m; i += kCsThreads) {
    b[0] = fmin(b[0], u[i]); b[1] = fmax(b[1], u[i]);
    b[2] = fmin(b[2], v[i]); b[3] = fmax(b[3], v[i]);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    b[0] = fmin(b[0], __shfl_xor(b[0], off, 64)); b[1] = fmax(b[1], __shfl_xor(b[1], off, 64));
    b[2] = fmin(b[2], __shfl_xor(b[2], off, 64)); b[3] = fmax(b[3], __shfl_xor(b[3], off, 64));
  }
  if ((threadIdx.x & 63) == 0)
    for (int k = 0; k < 4; ++k) lds[threadIdx.x >> 6][k] = b[k];
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int q = 1; q < kCsWaves; ++q) {
      b[0] = fmin(b[0], lds[q][0]); b[1] = fmax(b[1], lds[q][1]);
      b[2] = fmin(b[2], lds[q][2]); b[3] = fmax(b[3], lds[q][3]);
    }
    box[0] = b[0] - margin; box[1] = b[1] + margin; box[2] = b[2] - margin; box[3] = b[3] + margin;
    cnt[kCntTab] = 0;
    cnt[kCntPos] = 0;
    cnt[kCntErr] = INT_MAX;
  }
}

__global__ __launch_bounds__(kCsThreads) void k_cs_count(CsPts p, int n, CsParams a,
                                                          const double* __restrict__ box,
                                                          int32_t* __restrict__ blk_cnt) {
  __shared__ int s_c[kCsWaves][2];
  const int i = blockIdx.x * kCsThreads + threadIdx.x;
  bool pos = false, keep = false;
  if (i < n) {
    double pc[3], u, v;
    pos = cs_project(p, i, a, pc, &u, &v);
    keep = pos && cs_in_box(u, v, box);
  }
  const int ck = __popcll(__builtin_amdgcn_ballot_w64(keep)), cp = __popcll(__builtin_amdgcn_ballot_w64(pos));
  if ((threadIdx.x & 63) == 0) { s_c[threadIdx.x >> 6][0] = ck; s_c[threadIdx.x >> 6][1] = cp; }
  __syncthreads();
  if (threadIdx.x == 0) {
    int k = 0, q = 0;
    for (int w = 0; w < kCsWaves; ++w) { k += s_c[w][0]; q += s_c[w][1]; }
    blk_cnt[2 * blockIdx.x] = k;
    blk_cnt[2 * blockIdx.x + 1] = q;
  }
}

// exclusive scan of the blocks' kept counts (thread t owns a contiguous run of blocks); totals -> cnt
__global__ __launch_bounds__(kCsThreads) void k_cs_offsets(const int32_t* __restrict__ blk_cnt, int nblk,
                                                            int32_t* __restrict__ blk_off, int32_t* __restrict__ cnt) {
  __shared__ int s_w[kCsWaves][2];
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const int per = (nblk + kCsThreads - 1) / kCsThreads;
  const int b0 = min(nblk, t * per), b1 = min(nblk, b0 + per);
  int mine = 0, pos = 0;
  for (int b = b0; b < b1; ++b) { mine += blk_cnt[2 * b]; pos += blk_cnt[2 * b + 1]; }
  int x = mine;
  for (int off = 1; off < 64; off <<= 1) {
    const int y = __shfl_up(x, off, 64);
    if (lane >= off) x += y;
  }
  for (int off = 32; off >= 1; off >>= 1) pos += __shfl_xor(pos, off, 64);
  if (lane == 63) s_w[wid][0] = x;
  if (lane == 0) s_w[wid][1] = pos;
  __syncthreads();
  int run = x - mine;
  for (int q = 0; q < wid; ++q) run += s_w[q][0];
  for (int b = b0; b < b1; ++b) { blk_off[b] = run; run += blk_cnt[2 * b]; }
  if (t == 0) {
    int tot = 0, tp = 0;
    for (int q = 0; q < kCsWaves; ++q) { tot += s_w[q][0]; tp += s_w[q][1]; }
    cnt[kCntTab] = tot;
    cnt[kCntPos] = tp;
  }
}

// table rows: u | v | x | y | z, each a column of `cap` entries
__global__ __launch_bounds__(kCsThreads) void k_cs_compact(CsPts p, int n, CsParams a,
                                                            const double* __restrict__ box,
                                                            const int32_t* __restrict__ blk_off, double* __restrict__ tab,
                                                            int cap) {
  __shared__ int s_c[kCsWaves];
  const int i = blockIdx.x * kCsThreads + threadIdx.x, lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  bool keep = false;
  double pc[3], u = 0.0, v = 0.0;
  if (i < n) keep = cs_project(p, i, a, pc, &u, &v) && cs_in_box(u, v, box);
  const unsigned long long m = __builtin_amdgcn_ballot_w64(keep);
  if (lane == 0) s_c[wid] = __popcll(m);
  __syncthreads();
  if (!keep) return;
  int at = blk_off[blockIdx.x] + __popcll(m & ((1ull << lane) - 1ull));
  for (int w = 0; w < wid; ++w) at += s_c[w];
  if (at >= cap) return;   // cannot happen (at < n <= cap); keeps the stores inside the table
  tab[at] = u;
  tab[(size_t)cap + at] = v;
  tab[2 * (size_t)cap + at] = pc[0];
  tab[3 * (size_t)cap + at] = pc[1];
  tab[4 * (size_t)cap + at] = pc[2];
}

// sum over the workgroup in a fixed tree: lanes by xor shuffles, then the waves in order (every thread
// returns the same value)
__device__ __forceinline__ double cs_block_sum(double v, double* s_red) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  __syncthreads();   // s_red's previous readers
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = s_red[0];
  for (int q = 1; q < kCsWaves; ++q) s += s_red[q];
  return s;
}

__device__ __forceinline__ double cs_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// _softplus (:197-204)
__device__ __forceinline__ double cs_softplus(double x) {
  if (x > 20.0) return x;
  if (x < -20.0) return 0.0;
  return log(1.0 + exp(x));
}

// _sigmoid (:66-72)
__device__ __forceinline__ double cs_sigmoid(double x) {
  if (x >= 0.0) return 1.0 / (1.0 + exp(-x));
  const double t = exp(x);
  return t / (1.0 + t);
}

__global__ __launch_bounds__(kCsThreads) void k_cs_feature(const double* __restrict__ tab, int cap,
                                                            int32_t* __restrict__ cnt, CsParams a, CsIn in, int m,
                                                            CsOut o) {
  __shared__ int32_t s_idx[kCsMaxCand];
  __shared__ double s_z[kCsMaxCand], s_d[kCsMaxCand];
  __shared__ int32_t s_sel[kCsMaxFit];
  __shared__ int s_wc[kCsWaves];
  __shared__ double s_red[kCsWaves], s_pick[2], s_B[2];
  const int f = blockIdx.x, t = threadIdx.x, lane = t & 63, wid = t >> 6;
  if (f >= m) return;
  const int n_tab = min(cnt[kCntTab], cap), n_pos = cnt[kCntPos];
  const double uq = in.u[f], vq = in.v[f];
  const double* tu = tab;
  const double* tv = tab + (size_t)cap;
  const double* tx = tab + 2 * (size_t)cap;
  const double* ty = tab + 3 * (size_t)cap;
  const double* tz = tab + 4 * (size_t)cap;
  // ray_from_pixel (:172-180), normalised again as _distance_point_to_ray does (:189)
  double ray[3];
  {
    const double dx = (uq - a.cx) / a.fx, dy = (vq - a.cy) / a.fy;
    const double nr = sqrt(dx * dx + dy * dy + 1.0);
    if (nr < 1e-12) { ray[0] = 0.0; ray[1] = 0.0; ray[2] = 1.0; }
    else { ray[0] = dx / nr; ray[1] = dy / nr; ray[2] = 1.0 / nr; }
  }
  double rd[3];
  {
    const double nr = sqrt(ray[0] * ray[0] + ray[1] * ray[1] + ray[2] * ray[2]) + 1e-12;
    rd[0] = ray[0] / nr; rd[1] = ray[1] / nr; rd[2] = ray[2] / nr;
  }
  // candidates within the radius, in table (= point) order
  int n = 0;
  for (int base = 0; base < n_tab; base += kCsThreads) {
    const int e = base + t;
    bool ok = false;
    if (e < n_tab) {
      const double du = tu[e] - uq, dv = tv[e] - vq;
      ok = du * du + dv * dv <= a.r2;
    }
    const unsigned long long bal = __builtin_amdgcn_ballot_w64(ok);
    if (lane == 0) s_wc[wid] = __popcll(bal);
    __syncthreads();
    int at = n + __popcll(bal & ((1ull << lane) - 1ull));
    for (int w = 0; w < wid; ++w) at += s_wc[w];
    if (ok && at < a.max_cand) {
      const double x = tx[e], y = ty[e], z = tz[e];
      const double pl = x * rd[0] + y * rd[1] + z * rd[2];
      const double ex = x - pl * rd[0], ey = y - pl * rd[1], ez = z - pl * rd[2];
      s_idx[at] = e;
      s_z[at] = z;
      s_d[at] = ex * ex + ey * ey + ez * ez;
    }
    for (int w = 0; w < kCsWaves; ++w) n += s_wc[w];
    __syncthreads();
  }
  if (o.n_pt && t == 0) o.n_pt[f] = n;
  if (n > a.max_cand) {   // uniform: the call fails, k_cs_finish clears the batch rows
    if (t == 0) atomicMin(&cnt[kCntErr], f);
    return;
  }
  // ---- Route A (:137-162)
  double z_med = NAN, mad = NAN, Lam_A = 0.0, th_A = 0.0;
  const bool enough = n >= a.min_points && n >= 1;
  if (enough) {
    const int lo = (n - 1) / 2, hi = n / 2;   // np.median: the mean of the two middle order statistics
    for (int e = t; e < n; e += kCsThreads) {
      const double ze = s_z[e];
      int r = 0;
      for (int j = 0; j < n; ++j) {
        const double zj = s_z[j];
        r += (zj < ze || (zj == ze && j < e)) ? 1 : 0;
      }
      if (r == lo) s_pick[0] = ze;
      if (r == hi) s_pick[1] = ze;
    }
    __syncthreads();
    z_med = (s_pick[0] + s_pick[1]) / 2.0;
    __syncthreads();
    for (int e = t; e < n; e += kCsThreads) {
      const double ae = fabs(s_z[e] - z_med);
      int r = 0;
      for (int j = 0; j < n; ++j) {
        const double aj = fabs(s_z[j] - z_med);
        r += (aj < ae || (aj == ae && j < e)) ? 1 : 0;
      }
      if (r == lo) s_pick[0] = ae;
      if (r == hi) s_pick[1] = ae;
    }
    __syncthreads();
    mad = (s_pick[0] + s_pick[1]) / 2.0;
    double acc = 0.0;
    for (int e = t; e < n; e += kCsThreads) acc += s_z[e];
    const double mean = cs_block_sum(acc, s_red) / (double)n;
    acc = 0.0;
    for (int e = t; e < n; e += kCsThreads) { const double d = s_z[e] - mean; acc += d * d; }
    const double var_spread = n >= 2 ? cs_block_sum(acc, s_red) / (double)n : 0.0;
    const double sigma_A = kMadScale * mad, sigma_A_sq = sigma_A * sigma_A;
    double sig = a.base_sigma * a.base_sigma + fmax(sigma_A_sq, var_spread);
    sig = fmax(sig, a.var_min);
    const double w_cnt = cs_sigmoid(a.alpha_cnt * ((double)n - a.n0));
    const double w_mad = exp(-a.beta_mad * sigma_A_sq), w_repr = exp(-a.gamma_repr * var_spread);
    const double wA = w_cnt * w_mad * w_repr;
    if (wA > 0.0 && isfinite(z_med) && z_med > 0.0) {
      Lam_A = wA / sig;
      th_A = Lam_A * z_med;
    }
  }
  // ---- Route B (:276-348, :377-385): the k_use candidates nearest the ray, by (distance, position)
  if (t == 0) { s_B[0] = 0.0; s_B[1] = 0.0; }
  const bool route_b = enough && n_pos >= a.min_points;
  const int k_use = route_b ? min(min(a.fit_max, n_pos), n) : 0;
  if (route_b) {
    for (int e = t; e < n; e += kCsThreads) {
      const double de = s_d[e];
      int r = 0;
      for (int j = 0; j < n; ++j) {
        const double dj = s_d[j];
        r += (dj < de || (dj == de && j < e)) ? 1 : 0;
      }
      if (r < k_use) s_sel[r] = s_idx[e];
    }
  }
  __syncthreads();
  if (route_b && wid == 0) {   // _fit_plane_weighted (:207-239) with unit weights: lane l holds fitted point l
    const bool on = lane < k_use;
    double x = 0.0, y = 0.0, z = 0.0;
    if (on) { const int e = s_sel[lane]; x = tx[e]; y = ty[e]; z = tz[e]; }
    const double kn = (double)k_use;
    const double c0 = cs_wave_sum(x) / kn, c1 = cs_wave_sum(y) / kn, c2 = cs_wave_sum(z) / kn;
    const double d0 = on ? x - c0 : 0.0, d1 = on ? y - c1 : 0.0, d2 = on ? z - c2 : 0.0;
    const double wsum = kn + 1e-300;
    const double sxx = cs_wave_sum(d0 * d0) / wsum, sxy = cs_wave_sum(d0 * d1) / wsum, sxz = cs_wave_sum(d0 * d2) / wsum;
    const double syy = cs_wave_sum(d1 * d1) / wsum, syz = cs_wave_sum(d1 * d2) / wsum, szz = cs_wave_sum(d2 * d2) / wsum;
    const double S[9] = {sxx + 1e-12, sxy, sxz, sxy, syy + 1e-12, syz, sxz, syz, szz + 1e-12};
    double ev[3], V[9];
    eigh3_jacobi(S, ev, V);
    int i0 = 0, i1 = 1, i2 = 2;   // ascending
    if (ev[i1] < ev[i0]) { const int q = i0; i0 = i1; i1 = q; }
    if (ev[i2] < ev[i1]) { const int q = i1; i1 = i2; i2 = q; }
    if (ev[i1] < ev[i0]) { const int q = i0; i0 = i1; i1 = q; }
    double nrm[3] = {V[i0], V[3 + i0], V[6 + i0]};
    if (nrm[2] < 0.0) { nrm[0] = -nrm[0]; nrm[1] = -nrm[1]; nrm[2] = -nrm[2]; }
    const double res = d0 * nrm[0] + d1 * nrm[1] + d2 * nrm[2];
    const double sperp = fmax(cs_wave_sum(on ? res * res : 0.0) / kn, 0.0);
    const double nr = nrm[0] * ray[0] + nrm[1] * ray[1] + nrm[2] * ray[2];
    const double z_raw = (nrm[0] * c0 + nrm[1] * c1 + nrm[2] * c2) / (nr + a.delta);
    const double z_ell = cs_softplus(z_raw - a.z_min) + a.z_min;
    const double w_behind = z_raw < a.z_min ? cs_sigmoid(z_raw - a.z_min) : 1.0;
    const double nr_sq = nr * nr + a.delta;
    double sig = a.base_sigma * a.base_sigma + sperp / fmax(nr_sq, a.delta);
    sig = fmin(fmax(sig, a.var_min), a.sigma_max_sq);
    const double w_angle = cs_sigmoid(a.alpha_angle * (fabs(nr) - a.t_angle));
    const double lam2 = fmax(ev[i1], a.fit_eps), lam3 = fmax(ev[i2], a.fit_eps);
    const double rho = lam2 / (lam3 + a.fit_eps);
    const double w_planar = cs_sigmoid(a.beta_planar * (rho - a.rho0));
    const double w_res = exp(-a.gamma_res * sperp);
    const double w_z = cs_sigmoid(a.alpha_z * (z_ell - a.z_min));
    const double wB = fmax(w_angle * w_planar * w_res * w_behind * w_z, 0.0);
    if (lane == 0 && isfinite(z_ell) && z_ell > 0.0 && isfinite(sig) && sig > 0.0 && wB > 0.0) {
      const double s2 = fmax(sig, a.var_min);
      s_B[0] = wB / s2;
      s_B[1] = (wB / s2) * z_ell;
    }
  }
  __syncthreads();
  if (t != 0) return;
  const double Lam_B = s_B[0], th_B = s_B[1];
  // ---- lidar_depth_evidence's sum (:428-433) and the product of experts (splat_prep.py:73-93)
  double Lam_ell = Lam_A + Lam_B, th_ell = th_A + th_B;
  if (a.gamma != 1.0) { Lam_ell = Lam_ell * a.gamma; th_ell = th_ell * a.gamma; }
  const double Lam_f = a.w_cam * in.Lc[f] + a.w_lidar * Lam_ell;
  const double th_f = a.w_cam * in.thc[f] + a.w_lidar * th_ell;
  bool fused = !(Lam_f <= 0.0 || !isfinite(Lam_f) || !isfinite(th_f));
  double z_f = 0.0, var_f = 0.0;
  if (fused) {
    z_f = th_f / Lam_f;
    var_f = 1.0 / Lam_f;
    if (!isfinite(z_f) || z_f <= 0.0 || !isfinite(var_f) || var_f <= 0.0) fused = false;
  }
  if (o.z_med) o.z_med[f] = z_med;
  if (o.mad) o.mad[f] = mad;
  if (o.Lambda_A) o.Lambda_A[f] = Lam_A;
  if (o.theta_A) o.theta_A[f] = th_A;
  if (o.Lambda_B) o.Lambda_B[f] = Lam_B;
  if (o.theta_B) o.theta_B[f] = th_B;
  if (o.z_f) o.z_f[f] = fused ? z_f : 0.0;
  if (o.fused) o.fused[f] = fused ? 1 : 0;
  if (f >= a.n_feat) return;   // past the camera budget: diagnostics only
  double xyz[3], cov[9];
  if (fused) {   // backproject_camera / backprojection_cov_camera (:450-489)
    const double vz = fmax(fmax(var_f, a.var_min), 0.0), vu = fmax(a.pix_var, 0.0), vv = vu;
    const double du = uq - a.cx, dv = vq - a.cy;
    xyz[0] = du * z_f / a.fx;
    xyz[1] = dv * z_f / a.fy;
    xyz[2] = z_f;
    const double var_x = (z_f * z_f * vu + du * du * vz + vu * vz) / (a.fx * a.fx);
    const double var_y = (z_f * z_f * vv + dv * dv * vz + vv * vz) / (a.fy * a.fy);
    const double cxy = (du * dv * vz) / (a.fx * a.fy), cxz = (du * vz) / a.fx, cyz = (dv * vz) / a.fy;
    cov[0] = var_x; cov[1] = cxy; cov[2] = cxz;
    cov[3] = cxy; cov[4] = var_y; cov[5] = cyz;
    cov[6] = cxz; cov[7] = cyz; cov[8] = vz;
  } else {
    for (int q = 0; q < 3; ++q) xyz[q] = in.xyz[3 * (size_t)f + q];
    for (int q = 0; q < 9; ++q) cov[q] = in.cov[9 * (size_t)f + q];
  }
  // base frame (backend_node.py:1892-1899): R x + t, R Sigma R^T, R mu_app
  double xb[3], RS[9], Sb[9];
  for (int r = 0; r < 3; ++r) xb[r] = a.R[3 * r] * xyz[0] + a.R[3 * r + 1] * xyz[1] + a.R[3 * r + 2] * xyz[2] + a.t[r];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c)
      RS[3 * r + c] = a.R[3 * r] * cov[c] + a.R[3 * r + 1] * cov[3 + c] + a.R[3 * r + 2] * cov[6 + c];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c)
      Sb[3 * r + c] = RS[3 * r] * a.R[3 * c] + RS[3 * r + 1] * a.R[3 * c + 1] + RS[3 * r + 2] * a.R[3 * c + 2];
  double dir[3];
  if (in.has_mu[f]) {
    const double* mu = in.mu + 3 * (size_t)f;
    for (int r = 0; r < 3; ++r) dir[r] = a.R[3 * r] * mu[0] + a.R[3 * r + 1] * mu[1] + a.R[3 * r + 2] * mu[2];
  } else {
    for (int r = 0; r < 3; ++r) dir[r] = xb[r];
  }
  const double dn = sqrt(dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2]) + 1e-12;   // camera_batch_utils.py:64-65
  // measurement_batch_from_camera_splats (measurement_batch.py:203-243)
  double A[9], L[9];
  for (int q = 0; q < 9; ++q) A[q] = Sb[q];
  A[0] += a.eps_lift; A[4] += a.eps_lift; A[8] += a.eps_lift;
  inv3(A, L);
  const double kap = in.kappa[f];
  for (int q = 0; q < 9; ++q) o.Lambdas[9 * (size_t)f + q] = L[q];
  for (int q = 0; q < 3; ++q) o.thetas[3 * (size_t)f + q] = L[3 * q] * xb[0] + L[3 * q + 1] * xb[1] + L[3 * q + 2] * xb[2];
  for (int q = 0; q < 9; ++q) o.etas[9 * (size_t)f + q] = q < 3 ? kap * (dir[q] / dn) : 0.0;
  o.weights[f] = in.weight[f];
  o.sources[f] = 0;
  o.source_indices[f] = f;
  o.valid_mask[f] = 1;
  o.timestamps[f] = a.timestamp;
  for (int q = 0; q < 3; ++q)
    o.colors[3 * (size_t)f + q] = in.has_color[f] ? fmin(fmax(in.color[3 * (size_t)f + q], 0.0), 1.0) : 0.5;
}

// rows past n_valid: the empty batch's zeros; all rows when a feature overflowed.  status (mapped host
// memory): [0] n_camera_valid, [1] the first overflowing feature or INT_MAX
__global__ __launch_bounds__(kCsThreads) void k_cs_finish(const int32_t* __restrict__ cnt, int n_valid, int n_feat,
                                                           CsOut o, int32_t* __restrict__ status) {
  const int s = blockIdx.x * kCsThreads + threadIdx.x;
  const int err = cnt[kCntErr];
  if (s == 0) {
    status[0] = err == INT_MAX ? n_valid : 0;
    status[1] = err;
  }
  if (s >= n_feat || (err == INT_MAX && s < n_valid)) return;
  for (int q = 0; q < 9; ++q) o.Lambdas[9 * (size_t)s + q] = 0.0;
  for (int q = 0; q < 3; ++q) o.thetas[3 * (size_t)s + q] = 0.0;
  for (int q = 0; q < 9; ++q) o.etas[9 * (size_t)s + q] = 0.0;
  for (int q = 0; q < 3; ++q) o.colors[3 * (size_t)s + q] = 0.0;
  o.weights[s] = 0.0;
  o.timestamps[s] = 0.0;
  o.sources[s] = 0;
  o.source_indices[s] = 0;
  o.valid_mask[s] = 0;
}

}  // namespace
}  // namespace gcs

using namespace gcs;

struct gcs_camsplat_ctx {
  gcs_camsplat_config cfg{};
  std::string err;
  int device = 0;
  hipStream_t own = nullptr, stream = nullptr;
  double *d_tab = nullptr, *d_box = nullptr;
  int32_t *d_blk_cnt = nullptr, *d_blk_off = nullptr, *d_cnt = nullptr;
  int32_t* h_status = nullptr;      // pinned, mapped: written by k_cs_finish
  int32_t* h_status_dev = nullptr;
};

namespace {
int cs_fail(gcs_camsplat_ctx* c, int code, const std::string& m) {
  if (c) c->err = m;
  return code;
}
#define CSCHK(ctx, expr)                                                                          \
  do {                                                                                            \
    hipError_t _e = (expr);                                                                       \
    if (_e != hipSuccess) return cs_fail((ctx), GCS_ERR_HIP, std::string(#expr ": ") + hipGetErrorString(_e)); \
  } while (0)
}  // namespace

extern "C" {

int gcs_camsplat_config_defaults(gcs_camsplat_config* c) {
  if (!c) return GCS_ERR_ARG;
  memset(c, 0, sizeof(*c));
  c->depth_fusion_weight_camera = 1.0;   // lidar_camera_depth_fusion.py:34-63
  c->depth_fusion_weight_lidar = 1.0;
  c->gamma_lidar = 1.0;
  c->lidar_projection_radius_pix = 3.0;
  c->lidar_plane_fit_min_points = 3;
  c->lidar_depth_base_sigma_m = 0.02;
  c->lidar_incidence_sigma_scale = 1.0;
  c->depth_var_min_m2 = 1e-8;
  c->point_support_n0 = 3.0;
  c->point_support_alpha = 1.0;
  c->spread_mad_beta = 10.0;
  c->repr_gamma = 10.0;
  c->lidar_ray_plane_fit_max_points = 64;
  c->plane_intersection_delta = 1e-6;
  c->plane_angle_sigmoid_alpha = 10.0;
  c->plane_angle_sigmoid_t = 0.1;
  c->plane_planarity_sigmoid_beta = 5.0;
  c->plane_planarity_rho0 = 0.3;
  c->plane_residual_exp_gamma = 100.0;
  c->plane_fit_eps = 1e-12;
  c->depth_min_m = 0.05;
  c->depth_sigma_max_sq = 1e4;
  c->depth_min_sigmoid_alpha_z = 20.0;
  c->pixel_sigma = 1.0;    // splat_prep.py:43
  c->eps_lift = 1e-9;      // GC_EPS_LIFT, constants.py:71
  c->n_feat = 512;         // GC_N_FEAT, constants.py:350
  c->n_surfel = 1024;      // GC_N_SURFEL, constants.py:353
  c->max_points = 65536;
  c->max_candidates = kCsMaxCand;
  c->device = 0;
  return GCS_OK;
}

const char* gcs_camsplat_last_error(const gcs_camsplat_ctx* c) { return c ? c->err.c_str() : "null camera-splat context"; }

int gcs_camsplat_ctx_destroy(gcs_camsplat_ctx* c) {
  if (!c) return GCS_OK;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  void* bufs[] = {c->d_tab, c->d_box, c->d_blk_cnt, c->d_blk_off, c->d_cnt};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  if (c->h_status) (void)hipHostFree(c->h_status);
  if (c->own) (void)hipStreamDestroy(c->own);
  delete c;
  return GCS_OK;
}

int gcs_camsplat_ctx_create(const gcs_camsplat_config* cfg, gcs_camsplat_ctx** out) {
  if (!cfg || !out) return GCS_ERR_ARG;
  *out = nullptr;
  if (cfg->n_feat < 1 || cfg->n_surfel < 0 || cfg->max_points < 1 || cfg->max_candidates < 1 ||
      cfg->max_candidates > kCsMaxCand || cfg->lidar_ray_plane_fit_max_points < 1 ||
      cfg->lidar_ray_plane_fit_max_points > kCsMaxFit || cfg->lidar_plane_fit_min_points < 0 ||
      !(cfg->lidar_projection_radius_pix >= 0.0))
    return GCS_ERR_ARG;
  auto* c = new gcs_camsplat_ctx();
  c->cfg = *cfg;
  c->device = cfg->device;
  auto bad = [&](hipError_t e) { return e != hipSuccess; };
  const size_t N = (size_t)cfg->max_points, nblk = (N + kCsThreads - 1) / kCsThreads;
  if (bad(hipSetDevice(cfg->device)) || bad(hipStreamCreateWithFlags(&c->own, hipStreamNonBlocking)) ||
      bad(hipMalloc(&c->d_tab, 5 * N * sizeof(double))) || bad(hipMalloc(&c->d_box, 4 * sizeof(double))) ||
      bad(hipMalloc(&c->d_blk_cnt, 2 * nblk * 4)) || bad(hipMalloc(&c->d_blk_off, nblk * 4)) ||
      bad(hipMalloc(&c->d_cnt, 4 * 4)) || bad(hipHostMalloc(&c->h_status, 2 * 4, hipHostMallocMapped)) ||
      bad(hipHostGetDevicePointer((void**)&c->h_status_dev, c->h_status, 0))) {
    gcs_camsplat_ctx_destroy(c);
    return GCS_ERR_HIP;
  }
  c->stream = c->own;
  *out = c;
  return GCS_OK;
}

int gcs_camsplat_ctx_set_stream(gcs_camsplat_ctx* c, void* stream) {
  if (!c) return GCS_ERR_ARG;
  hipStream_t ns = stream ? (hipStream_t)stream : c->own;
  if (ns == c->stream) return GCS_OK;
  CSCHK(c, hipSetDevice(c->device));
  CSCHK(c, hipStreamSynchronize(c->stream));  // work queued on the old stream completes first
  c->stream = ns;
  return GCS_OK;
}

}  // extern "C"

namespace gcs {
namespace live {
int camsplat_bind_stream(gcs_camsplat_ctx* c, void* s) {
  if ((hipStream_t)s == c->stream) return GCS_OK;
  CSCHK(c, hipSetDevice(c->device));
  CSCHK(c, hipStreamSynchronize(c->stream));
  c->stream = (hipStream_t)s;
  return GCS_OK;
}

int camsplat_launch(gcs_camsplat_ctx* c, const gcs_camsplat_inputs* in, const void* xyz, int32_t point_step,
                    int32_t xyz_format, int32_t n_points, gcs_camsplat_outputs* out, int32_t* n_valid_host) {
  if (!c || !in || !out) return GCS_ERR_ARG;
  const gcs_camsplat_config& cf = c->cfg;
  const int n = n_points, m = in->n_features;
  if (n < 0 || n > cf.max_points) return cs_fail(c, GCS_ERR_ARG, "n_points exceeds max_points");
  if (m < 0 || m > 65535) return cs_fail(c, GCS_ERR_ARG, "n_features out of range");
  if (n > 0 && !xyz) return cs_fail(c, GCS_ERR_ARG, "null points");
  if (xyz_format == 0 ? (point_step < 12 || point_step % 4 != 0) : (xyz_format != 1 || point_step < 24 || point_step % 8 != 0))
    return cs_fail(c, GCS_ERR_ARG, "xyz_format 0 needs a point_step >= 12 (a multiple of 4), xyz_format 1 one >= 24 "
                                   "(a multiple of 8)");
  if (m > 0 && (!in->u || !in->v || !in->depth_Lambda_c || !in->depth_theta_c || !in->xyz || !in->cov ||
                !in->weight || !in->kappa_app || !in->mu_app || !in->has_mu || !in->color || !in->has_color))
    return cs_fail(c, GCS_ERR_ARG, "null feature array");
  if (!out->Lambdas || !out->thetas || !out->etas || !out->weights || !out->sources || !out->source_indices ||
      !out->valid_mask || !out->timestamps || !out->colors)
    return cs_fail(c, GCS_ERR_ARG, "null batch array");
  CSCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  CsParams a{};
  for (int k = 0; k < 9; ++k) a.R[k] = in->R_base_camera[k];
  for (int k = 0; k < 3; ++k) a.t[k] = in->t_base_camera[k];
  a.fx = in->fx; a.fy = in->fy; a.cx = in->cx; a.cy = in->cy;
  a.w_cam = cf.depth_fusion_weight_camera; a.w_lidar = cf.depth_fusion_weight_lidar; a.gamma = cf.gamma_lidar;
  const double r = cf.lidar_projection_radius_pix;
  a.r2 = r * r;
  a.base_sigma = cf.lidar_depth_base_sigma_m; a.var_min = cf.depth_var_min_m2;
  a.n0 = cf.point_support_n0; a.alpha_cnt = cf.point_support_alpha;
  a.beta_mad = cf.spread_mad_beta; a.gamma_repr = cf.repr_gamma;
  a.delta = cf.plane_intersection_delta; a.alpha_angle = cf.plane_angle_sigmoid_alpha;
  a.t_angle = cf.plane_angle_sigmoid_t; a.beta_planar = cf.plane_planarity_sigmoid_beta;
  a.rho0 = cf.plane_planarity_rho0; a.gamma_res = cf.plane_residual_exp_gamma; a.fit_eps = cf.plane_fit_eps;
  a.z_min = cf.depth_min_m; a.sigma_max_sq = cf.depth_sigma_max_sq; a.alpha_z = cf.depth_min_sigmoid_alpha_z;
  a.pix_var = cf.pixel_sigma * cf.pixel_sigma; a.eps_lift = cf.eps_lift; a.timestamp = in->timestamp_sec;
  // the box holds every pixel within the radius of a query: a little wider than r, so the rounding of
  // the test's squares and of the box's own corners cannot cut a candidate
  a.box_margin = r * (1.0 + 1e-6) + 1e-6;
  a.min_points = cf.lidar_plane_fit_min_points; a.fit_max = cf.lidar_ray_plane_fit_max_points;
  a.max_cand = cf.max_candidates; a.n_feat = cf.n_feat;
  CsIn ci{in->u, in->v, in->depth_Lambda_c, in->depth_theta_c, in->xyz, in->cov, in->weight, in->kappa_app,
          in->mu_app, in->color, in->has_mu, in->has_color};
  CsOut co{out->Lambdas, out->thetas, out->etas, out->weights, out->timestamps, out->colors, out->sources,
           out->source_indices, out->valid_mask, out->n_pt, out->z_med, out->mad, out->Lambda_A, out->theta_A,
           out->Lambda_B, out->theta_B, out->z_f, out->fused};
  const int n_valid = std::min(m, cf.n_feat);
  const CsPts pts{xyz, point_step, xyz_format};
  hipLaunchKernelGGL(k_cs_box, dim3(1), dim3(kCsThreads), 0, s, in->u, in->v, m, a.box_margin, c->d_box, c->d_cnt);
  if (m > 0) {
    if (n > 0) {
      const int nblk = (n + kCsThreads - 1) / kCsThreads;
      hipLaunchKernelGGL(k_cs_count, dim3(nblk), dim3(kCsThreads), 0, s, pts, n, a, (const double*)c->d_box,
                         c->d_blk_cnt);
      hipLaunchKernelGGL(k_cs_offsets, dim3(1), dim3(kCsThreads), 0, s, (const int32_t*)c->d_blk_cnt, nblk,
                         c->d_blk_off, c->d_cnt);
      hipLaunchKernelGGL(k_cs_compact, dim3(nblk), dim3(kCsThreads), 0, s, pts, n, a, (const double*)c->d_box,
                         (const int32_t*)c->d_blk_off, c->d_tab, cf.max_points);
    }
    hipLaunchKernelGGL(k_cs_feature, dim3(m), dim3(kCsThreads), 0, s, (const double*)c->d_tab, cf.max_points,
                       c->d_cnt, a, ci, m, co);
  }
  hipLaunchKernelGGL(k_cs_finish, dim3((cf.n_feat + kCsThreads - 1) / kCsThreads), dim3(kCsThreads), 0, s,
                     (const int32_t*)c->d_cnt, n_valid, cf.n_feat, co, c->h_status_dev);
  CSCHK(c, hipGetLastError());
  if (n_valid_host) *n_valid_host = n_valid;
  return GCS_OK;
}

// after the stream's wait: k_cs_finish's status -- n_camera_valid and the first feature over max_candidates
int camsplat_collect(gcs_camsplat_ctx* c, gcs_camsplat_outputs* out) {
  out->n_camera_valid = c->h_status[0];
  if (c->h_status[1] != INT_MAX)
    return cs_fail(c, GCS_ERR_STATE, "feature " + std::to_string(c->h_status[1]) + " has more than max_candidates=" +
                                         std::to_string(c->cfg.max_candidates) +
                                         " LiDAR points within lidar_projection_radius_pix; no camera row was written");
  return GCS_OK;
}
}  // namespace live
}  // namespace gcs

extern "C" {

int gcs_camera_splats(gcs_camsplat_ctx* c, const gcs_camsplat_inputs* in, gcs_camsplat_outputs* out) {
  if (!c || !in || !out) return GCS_ERR_ARG;
  if (int rc = gcs::live::camsplat_launch(c, in, in->points_base, 24, 1, in->n_points, out, nullptr)) return rc;
  CSCHK(c, hipStreamSynchronize(c->stream));
  return gcs::live::camsplat_collect(c, out);
}

int gcs_camera_splats_scan(gcs_camsplat_ctx* c, const gcs_camsplat_inputs* in, const void* xyz_dev, int32_t point_step,
                           int32_t xyz_format, int32_t n_points, gcs_camsplat_outputs* out) {
  if (!c || !in || !out) return GCS_ERR_ARG;
  if (int rc = gcs::live::camsplat_launch(c, in, xyz_dev, point_step, xyz_format, n_points, out, nullptr)) return rc;
  CSCHK(c, hipStreamSynchronize(c->stream));
  return gcs::live::camsplat_collect(c, out);
}

}  // extern "C"
