// Per-keypoint math of the visual feature operator (visual_feature_node.cpp:228-652), shared by the
// device kernel (gcs_visfeat.hip, one wave64 per keypoint, one lane per window pixel) and the host
// build of the same rows (gcs_visual_features_host, which steps 64 lanes in a loop).  The per-lane
// pieces (window offsets, the depth load, the rank order of the median, a row of the normal equations)
// and the per-keypoint tail (the 6 x 6 SPD solve, curvature, variances, covariance, weights) live
// here; the cross-lane steps are a rank count and a butterfly sum whose order both builds repeat:
// for off = 32, 16, ..., 1: x[lane] += x[lane ^ off].  All f64, nothing contracted into an fma.
#pragma once

#include <math.h>
#include <stdint.h>

#include "gcs_math.h"
#include "gcslam_hip.h"

#pragma clang fp contract(off)

namespace gcs {

constexpr int kVfLanes = 64;
constexpr int kVfSums = 27;       // 21 entries of the symmetric A^T A (upper triangle, row-major) + 6 of A^T b
constexpr double kVfEps = 1e-12;  // kEps (:34)

struct VfImage {
  const void* depth;      // format 0: float32, 1: uint16
  const uint8_t* rgb;     // rgb8 or null
  int64_t depth_pitch, rgb_pitch;   // bytes per row
  int32_t depth_format, width, height;
};

struct VfParams {
  int32_t mode, model, quad_r, quad_min_points, n_sample_lanes;
  int32_t hex_dx[7], hex_dy[7];   // centre, then round(r cos(k pi / 3)), round(r sin(k pi / 3)) (:303-312), from the host
  double fx, fy, cx, cy;
  double pixel_sigma, depth_sigma0, depth_sigma_slope, min_depth_m, max_depth_m, depth_validity_slope;
  double response_soft_scale, depth_scale, invalid_cov_inflate, quad_fit_lstsq_eps;
  double student_t_nu, student_t_w_min, ma_tau, ma_delta_inflate, kappa0, kappa_alpha, kappa_max, kappa_min;
};

// What the cross-lane steps hand to the tail.
struct VfKeypoint {
  double u, v, response;
  int32_t kp_index;
  bool z_valid;          // depth_sample's result (:552)
  int32_t n_depth;       // valid values in the depth sample (zs.size(); nearest: 0 or 1)
  int32_t n_zs;          // the zs the Student-t step sees (nearest: 0, :240-244)
  double z_m, z_var;     // z_var NaN where the node has none
  double q_sum;          // sum (zi - z_m)^2 over the sample
  int32_t n_fit;         // valid pixels of the fit window (0 when the depth is invalid: the fit is not run)
  double sums[kVfSums];  // A^T A (without the eps) and A^T b
};

// static_cast<int>(std::round(x)): half away from zero.  |x| <= 1e9 here.
GCS_HD int vf_round(double x) { return (int)round(x); }

// clamp (:46-49) with std::min / std::max's NaN behaviour: a NaN v gives hi
GCS_HD double vf_clamp(double v, double lo, double hi) {
  const double m = (v < hi) ? v : hi;
  return (lo < m) ? m : lo;
}

// Declared: a non-finite coordinate, or one beyond 1e9 in magnitude, is outside the image.
GCS_HD bool vf_pixel(double u, double v, const VfImage& im, int* x, int* y) {
  *x = *y = 0;
  if (!(isfinite(u) && isfinite(v)) || fabs(u) > 1e9 || fabs(v) > 1e9) return false;
  *x = vf_round(u);
  *y = vf_round(v);
  return *x >= 0 && *y >= 0 && *x < im.width && *y < im.height;
}

// depth_to_meters of pixel (xi, yi); false outside the image or where the value is not finite and > 0
GCS_HD bool vf_depth_at(const VfImage& im, double depth_scale, int xi, int yi, double* z) {
  *z = 0.0;
  if (xi < 0 || yi < 0 || xi >= im.width || yi >= im.height) return false;
  const uint8_t* row = (const uint8_t*)im.depth + (size_t)yi * (size_t)im.depth_pitch;
  const double raw = im.depth_format == 1 ? (double)((const uint16_t*)row)[xi] : (double)((const float*)row)[xi];
  const double zm = raw * depth_scale;
  if (!(isfinite(zm) && zm > 0.0)) return false;
  *z = zm;
  return true;
}

// lane -> offset within the depth sample's window (raster order, :266-267; hex: the tap list)
GCS_HD bool vf_sample_offset(const VfParams& p, int lane, int* dx, int* dy) {
  *dx = *dy = 0;
  if (lane >= p.n_sample_lanes) return false;
  if (p.mode == GCS_VF_HEX) {
    *dx = p.hex_dx[lane];
    *dy = p.hex_dy[lane];
  } else if (p.mode != GCS_VF_NEAREST) {
    const int r = p.mode == GCS_VF_MEDIAN3 ? 1 : 2, w = 2 * r + 1;
    *dx = lane % w - r;
    *dy = lane / w - r;
  }
  return true;
}

// lane -> offset within the fit's (2r + 1)^2 window (raster order, :410-411)
GCS_HD bool vf_fit_offset(const VfParams& p, int lane, int* dx, int* dy) {
  const int w = 2 * p.quad_r + 1;
  *dx = lane % w - p.quad_r;
  *dy = lane / w - p.quad_r;
  return lane < w * w;
}

// the strict order of the rank count: by value, ties by lane
GCS_HD bool vf_before(double zj, int j, double zi, int i) { return zj < zi || (zj == zi && j < i); }

// one pixel's terms of A^T A and A^T b (:430-444): row (ut^2, ut vt, vt^2, ut, vt, 1)
GCS_HD void vf_fit_terms(double ut, double vt, double z, double* t) {
  const double a[6] = {ut * ut, ut * vt, vt * vt, ut, vt, 1.0};
  int k = 0;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) t[k++] = a[i] * a[j];
  for (int i = 0; i < 6; ++i) t[k++] = a[i] * z;
}

// Cholesky solve of the 6 x 6 SPD system (M + eps I) beta = rhs; M: upper triangle, row-major
GCS_HD void vf_solve6(const double* sums, double eps, double* beta) {
  double Lm[6][6];
  int k = 0;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) {
      Lm[j][i] = sums[k++];
      if (i == j) Lm[i][i] += eps;
    }
  for (int j = 0; j < 6; ++j) {
    double d = Lm[j][j];
    for (int q = 0; q < j; ++q) d -= Lm[j][q] * Lm[j][q];
    d = sqrt(d);
    Lm[j][j] = d;
    for (int i = j + 1; i < 6; ++i) {
      double s = Lm[i][j];
      for (int q = 0; q < j; ++q) s -= Lm[i][q] * Lm[j][q];
      Lm[i][j] = s / d;
    }
  }
  double y[6];
  for (int i = 0; i < 6; ++i) {
    double s = sums[21 + i];
    for (int q = 0; q < i; ++q) s -= Lm[i][q] * y[q];
    y[i] = s / Lm[i][i];
  }
  for (int i = 5; i >= 0; --i) {
    double s = y[i];
    for (int q = i + 1; q < 6; ++q) s -= Lm[q][i] * beta[q];
    beta[i] = s / Lm[i][i];
  }
}

GCS_HD double vf_safe_sigmoid(double x) {   // :37-44
  if (x >= 0.0) return 1.0 / (1.0 + exp(-x));
  const double ex = exp(x);
  return ex / (1.0 + ex);
}

GCS_HD double vf_depth_sigma(const VfParams& p, double z_m) {   // :216-226
  const double z = fabs(z_m);
  return p.depth_sigma0 + p.depth_sigma_slope * (p.model == GCS_VF_DEPTH_QUADRATIC ? z * z : z);
}

// The tail of on_rgbd's loop body (:552-641) and _feature_batch_to_list (backend_node.py:1589-1650) for one
// keypoint, written to row `row` of the outputs.
GCS_HD void vf_finish(const VfParams& p, const VfImage& im, const VfKeypoint& k, int row,
                      const gcs_visfeat_outputs& o) {
  const double nan = NAN;
  const double u = k.u, v = k.v, z = k.z_m;
  const bool zv = k.z_valid;

  // weights (:196-214, :554-556); declared: a NaN response weighs 0
  double w_depth = 0.0;
  if (zv) {
    const double a = p.depth_validity_slope;
    const double w_lo = 1.0 / (1.0 + exp(-a * (z - p.min_depth_m)));
    const double w_hi = 1.0 / (1.0 + exp(+a * (z - p.max_depth_m)));
    w_depth = vf_clamp(w_lo * w_hi, 0.0, 1.0);
  }
  const double w_resp = (k.response > 0.0) ? k.response / (k.response + p.response_soft_scale) : 0.0;
  const double weight = vf_clamp(w_depth * w_resp, 0.0, 1.0);

  // quadratic fit (:423-490)
  const bool fit = zv && k.n_fit >= p.quad_min_points;
  double beta[6] = {nan, nan, nan, nan, nan, nan}, K = nan, lam_min = nan, w_ma = nan, normal[3] = {0.0, 0.0, 0.0};
  if (fit) {
    vf_solve6(k.sums, p.quad_fit_lstsq_eps, beta);
    const double zc = fmax(z, 1e-6);
    const double sx = p.fx / zc, sy = p.fy / zc;
    const double zu = sx * beta[3], zvp = sy * beta[4];
    const double h00 = sx * sx * (2.0 * beta[0]), h01 = sx * sy * beta[1], h11 = sy * sy * (2.0 * beta[2]);
    const double det = h00 * h11 - h01 * h01;
    const double denom = 1.0 + (zu * zu + zvp * zvp);
    K = (denom > 0.0) ? det / (denom * denom) : 0.0;
    const double hd = 0.5 * (h00 - h11);
    lam_min = 0.5 * (h00 + h11) - sqrt(hd * hd + h01 * h01);
    w_ma = vf_safe_sigmoid(p.ma_tau * lam_min);
    normal[0] = -zu; normal[1] = -zvp; normal[2] = 1.0;
    const double nn = sqrt(normal[0] * normal[0] + normal[1] * normal[1] + normal[2] * normal[2]);
    if (nn > 0.0)
      for (int j = 0; j < 3; ++j) normal[j] /= nn;
  }

  // effective depth variance (:563-572, :350-369)
  double var_z_eff = nan, sig2 = nan;
  if (zv) {
    const double s = vf_depth_sigma(p, z);
    sig2 = s * s;
    if (isfinite(k.z_var)) {
      const double base = fmax(k.z_var, sig2);
      var_z_eff = base;
      if (k.n_zs >= 2 && isfinite(base) && base > 0.0) {
        const double sigma2 = fmax(base, kVfEps);
        const double q = k.q_sum / ((double)k.n_zs * sigma2 + kVfEps);
        double w = (p.student_t_nu + 1.0) / (p.student_t_nu + q);
        if (w < p.student_t_w_min) w = p.student_t_w_min;
        var_z_eff = base / w;
      }
    } else {
      var_z_eff = sig2;
    }
    if (!isfinite(var_z_eff)) var_z_eff = sig2;
  }

  // back-projection and covariance (:371-399, :574-585)
  double xyz[3] = {0.0, 0.0, 0.0}, cov[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  cov[0] = cov[4] = cov[8] = p.invalid_cov_inflate;
  if (zv) {
    xyz[0] = (u - p.cx) * z / p.fx;
    xyz[1] = (v - p.cy) * z / p.fy;
    xyz[2] = z;
    const double du = u - p.cx, dv = v - p.cy;
    const double vu = fmax(p.pixel_sigma * p.pixel_sigma, 0.0), vv = vu;
    const double vz = fmax(fmax(var_z_eff, sig2), 0.0);
    cov[0] = (z * z * vu + du * du * vz + vu * vz) / (p.fx * p.fx);
    cov[4] = (z * z * vv + dv * dv * vz + vv * vz) / (p.fy * p.fy);
    cov[8] = vz;
    cov[1] = cov[3] = (du * dv * vz) / (p.fx * p.fy);
    cov[2] = cov[6] = (du * vz) / p.fx;
    cov[5] = cov[7] = (dv * vz) / p.fy;
    if (fit) {
      const double add = (1.0 - w_ma) * p.ma_delta_inflate;
      cov[0] += add; cov[4] += add; cov[8] += add;
    }
  }

  // vMF appearance (:587-600) and _feature_batch_to_list's second normalisation (backend_node.py:1616-1620)
  double mu[3] = {0.0, 0.0, 0.0}, kappa = 0.0;
  if (fit) {
    const double rel = (zv && isfinite(var_z_eff)) ? sqrt(var_z_eff) / (z + kVfEps) : 1.0;
    const double rho = 1.0 / (rel + kVfEps);
    kappa = p.kappa0 + p.kappa_alpha * sqrt(fabs(K)) * rho;
    kappa = vf_clamp(kappa, p.kappa_min, p.kappa_max) * w_ma;
    const double nn = sqrt(normal[0] * normal[0] + normal[1] * normal[1] + normal[2] * normal[2]) + 1e-12;
    for (int j = 0; j < 3; ++j) mu[j] = normal[j] / nn;
  }

  double lam_c = 0.0, th_c = 0.0;   // :602-609
  if (zv && isfinite(var_z_eff) && var_z_eff > 0.0) {
    lam_c = 1.0 / var_z_eff;
    th_c = lam_c * z;
  }

  double col[3] = {0.0, 0.0, 0.0};   // :611-616
  if (im.rgb) {
    const int ix = vf_round(vf_clamp(u, 0.0, (double)(im.width - 1)));
    const int iy = vf_round(vf_clamp(v, 0.0, (double)(im.height - 1)));
    const uint8_t* px = im.rgb + (size_t)iy * (size_t)im.rgb_pitch + 3 * (size_t)ix;
    for (int j = 0; j < 3; ++j) col[j] = (double)px[j] / 255.0;
  }

  const size_t r = (size_t)row;
  o.u[r] = u; o.v[r] = v;
  for (int j = 0; j < 3; ++j) o.xyz[3 * r + j] = xyz[j];
  for (int j = 0; j < 9; ++j) o.cov[9 * r + j] = cov[j];
  o.weight[r] = weight;
  o.kappa_app[r] = kappa;
  for (int j = 0; j < 3; ++j) o.mu_app[3 * r + j] = mu[j];
  o.has_mu[r] = fit ? 1 : 0;
  for (int j = 0; j < 3; ++j) o.color[3 * r + j] = col[j];
  o.has_color[r] = im.rgb ? 1 : 0;
  o.depth_Lambda_c[r] = lam_c;
  o.depth_theta_c[r] = th_c;
  if (o.kp_index) o.kp_index[r] = k.kp_index;
  if (o.z_valid) o.z_valid[r] = zv ? 1 : 0;
  if (o.n_depth) o.n_depth[r] = k.n_depth;
  if (o.n_fit) o.n_fit[r] = k.n_fit;
  if (o.z_m) o.z_m[r] = zv ? z : nan;
  if (o.z_var) o.z_var[r] = zv ? k.z_var : nan;
  if (o.var_z_eff) o.var_z_eff[r] = var_z_eff;
  if (o.beta)
    for (int j = 0; j < 6; ++j) o.beta[6 * r + j] = beta[j];
  if (o.K) o.K[r] = K;
  if (o.lam_min) o.lam_min[r] = lam_min;
  if (o.w_ma) o.w_ma[r] = w_ma;
}

// Rows [count, max_features): zeros (kp_index -1).
GCS_HD void vf_zero_row(int row, const gcs_visfeat_outputs& o) {
  const size_t r = (size_t)row;
  o.u[r] = o.v[r] = o.weight[r] = o.kappa_app[r] = o.depth_Lambda_c[r] = o.depth_theta_c[r] = 0.0;
  for (int j = 0; j < 3; ++j) o.xyz[3 * r + j] = o.mu_app[3 * r + j] = o.color[3 * r + j] = 0.0;
  for (int j = 0; j < 9; ++j) o.cov[9 * r + j] = 0.0;
  o.has_mu[r] = o.has_color[r] = 0;
  if (o.kp_index) o.kp_index[r] = -1;
  if (o.z_valid) o.z_valid[r] = 0;
  if (o.n_depth) o.n_depth[r] = 0;
  if (o.n_fit) o.n_fit[r] = 0;
  if (o.z_m) o.z_m[r] = 0.0;
  if (o.z_var) o.z_var[r] = 0.0;
  if (o.var_z_eff) o.var_z_eff[r] = 0.0;
  if (o.beta)
    for (int j = 0; j < 6; ++j) o.beta[6 * r + j] = 0.0;
  if (o.K) o.K[r] = 0.0;
  if (o.lam_min) o.lam_min[r] = 0.0;
  if (o.w_ma) o.w_ma[r] = 0.0;
}

// Selection order (declared): larger response first, NaN last, ties to the lower index.
GCS_HD bool vf_resp_before(float rj, int j, float ri, int i) {
  const float a = (rj == rj) ? rj : -INFINITY, b = (ri == ri) ? ri : -INFINITY;
  return a > b || (a == b && j < i);
}

}  // namespace gcs
