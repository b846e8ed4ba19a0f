// Per-splat math of the map renderer, shared by the device kernels (gcs_render.hip) and the host
// build of the same rows (gcs_render_prepare_host): the BEV pushforward (common/bev_pushforward.py:42-64),
// opacity from precision (backend/rendering.py:236-244), one-lobe vMF shading (:117-159, the form
// tools/build_rerun_from_splat.py:151-176 calls it in) and the hash value-noise fBm (:167-228).
// Everything here feeds the binning's integer decisions or has to repeat the reference's f64
// operation order, so nothing is contracted into an fma.
#pragma once

#include <math.h>
#include <stdint.h>

#include "gcs_math.h"

#pragma clang fp contract(off)

namespace gcs {

struct RnParams {
  double gamma, logdet0, alpha_min, eps;        // opacity_from_logdet and the radius floor
  double int_scale, int_max, kappa_max;         // kappa_modulated_by_intensity
  double fbm_gain, fbm_scale;
  int32_t fbm_octaves;
  int64_t fbm_seed;
};

// vmf_shading_multi_lobe's and kappa_modulated_by_intensity's own eps (rendering.py:102,126): the composed
// call leaves it at its default, whatever the config's eps (the radius floor of splat_indices_for_tile) is.
constexpr double kRnNormEps = 1e-12;

// rendering.py:167-170.  Python's integers do not wrap; the masks keep the low 31 bits, which
// two's-complement wrap-around leaves untouched, so unsigned 64-bit arithmetic gives the same value.
GCS_HD double rn_hash_float(uint64_t h) {
  h = (h * 1103515245ull + 12345ull) & 0x7FFFFFFFull;
  return (double)(int64_t)h / 2147483648.0;
}

GCS_HD double rn_value_noise_2d(double x, double y, int64_t seed) {   // :173-188
  const double flx = floor(x), fly = floor(y);
  const uint64_t ix = (uint64_t)(int64_t)flx, iy = (uint64_t)(int64_t)fly;
  double fx = x - flx, fy = y - fly;
  fx = fmax(0.0, fmin(1.0, fx));
  fy = fmax(0.0, fmin(1.0, fy));
  const uint64_t s31 = (uint64_t)seed * 31ull;
  const double v00 = rn_hash_float(((s31 + ix) * 31ull + iy) & 0x7FFFFFFFull);
  const double v10 = rn_hash_float(((s31 + ix + 1ull) * 31ull + iy) & 0x7FFFFFFFull);
  const double v01 = rn_hash_float(((s31 + ix) * 31ull + iy + 1ull) & 0x7FFFFFFFull);
  const double v11 = rn_hash_float(((s31 + ix + 1ull) * 31ull + iy + 1ull) & 0x7FFFFFFFull);
  const double sx = fx * fx * (3.0 - 2.0 * fx);
  const double sy = fy * fy * (3.0 - 2.0 * fy);
  const double v0 = v00 * (1.0 - sx) + v10 * sx;
  const double v1 = v01 * (1.0 - sx) + v11 * sx;
  return v0 * (1.0 - sy) + v1 * sy;
}

GCS_HD double rn_fbm(double x, double y, int octaves, double gain, int64_t seed) {   // :191-209
  double value = 0.0, amplitude = 1.0, frequency = 1.0, max_amplitude = 0.0;
  for (int o = 0; o < octaves; ++o) {
    value += amplitude * rn_value_noise_2d(x * frequency, y * frequency, seed);
    max_amplitude += amplitude;
    amplitude *= gain;
    frequency *= 2.0;
  }
  return value / (max_amplitude + 1e-12);
}

GCS_HD double rn_opacity(double logdet, double gamma, double logdet0, double alpha_min) {   // :236-244
  const double raw = 1.0 / (1.0 + exp(-gamma * (logdet0 - logdet)));
  return alpha_min + (1.0 - alpha_min) * raw;
}

// log det of a symmetric 3 x 3 by LDL^T (lower triangle read): the pivots' product loses nothing to
// the cancellation a cofactor expansion has on a thin covariance.  NaN where it is not positive definite.
GCS_HD double rn_logdet3(const double* S) {
  const double d0 = S[0];
  const double l10 = S[3] / d0, l20 = S[6] / d0;
  const double d1 = S[4] - l10 * S[3];
  const double l21 = (S[7] - l20 * S[3]) / d1;
  const double d2 = S[8] - l20 * S[6] - l21 * (l21 * d1);
  if (!(d0 > 0.0) || !(d1 > 0.0) || !(d2 > 0.0)) return NAN;
  return log(d0 * d1 * d2);
}

GCS_HD double rn_kappa_modulated(double kappa, double intensity, const RnParams& a) {   // :96-114
  if (a.int_scale <= 0.0 || a.int_max <= kRnNormEps) return kappa;
  double t = intensity / fmax(a.int_max, kRnNormEps);
  t = fmax(0.0, fmin(1.0, t));
  return fmin(kappa * (1.0 + a.int_scale * t), a.kappa_max);
}

// vmf_shading_multi_lobe with one lobe and uniform pi (= 1): exp(k (mu . v - 1)) / (1 + k).
// vn: the view direction already divided by (|v| + kRnNormEps).
GCS_HD double rn_shade_one_lobe(const double* vn, const double* dir, double kappa, bool has_int, double intensity,
                                const RnParams& a) {
  const double nrm = sqrt(dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2]) + kRnNormEps;
  const double m0 = dir[0] / nrm, m1 = dir[1] / nrm, m2 = dir[2] / nrm;
  double k = kappa;
  if (a.int_scale > 0.0 && has_int) k = rn_kappa_modulated(k, intensity, a);
  const double s = exp(k * ((m0 * vn[0] + m1 * vn[1] + m2 * vn[2]) - 1.0));
  return s / (1.0 + k);
}

// lambda_min of the symmetric 2 x 2 [[a, b], [b, c]] (eigvalsh reads the lower triangle) and the
// binning radius 2 / sqrt(max(lambda_min, eps)) (rendering.py:279-281).
GCS_HD double rn_radius(double a, double b, double c, double eps) {
  const double h = 0.5 * (a - c);
  const double lam = 0.5 * (a + c) - sqrt(h * h + b * b);
  return 2.0 / sqrt(fmax(lam, eps));
}

// One view of one row: mu' = P p + off, Sigma' = P Sigma P^T, its adjugate inverse, the radius.
// P: 2 x 3 row-major.  Returns false (and writes nothing) where Sigma' is not invertible to finite values.
GCS_HD bool rn_push_row(const double* p, const double* S, const double* P, const double* off, double eps,
                        double* mu2, double* Sinv, double* r) {
  double PS[6];
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 3; ++j)
      PS[3 * i + j] = (P[3 * i] * S[j] + P[3 * i + 1] * S[3 + j]) + P[3 * i + 2] * S[6 + j];
  const double s00 = (PS[0] * P[0] + PS[1] * P[1]) + PS[2] * P[2];
  const double s01 = (PS[0] * P[3] + PS[1] * P[4]) + PS[2] * P[5];
  const double s10 = (PS[3] * P[0] + PS[4] * P[1]) + PS[5] * P[2];
  const double s11 = (PS[3] * P[3] + PS[4] * P[4]) + PS[5] * P[5];
  const double det = s00 * s11 - s01 * s10;
  const double i00 = s11 / det, i01 = -s01 / det, i10 = -s10 / det, i11 = s00 / det;
  const double m0 = ((P[0] * p[0] + P[1] * p[1]) + P[2] * p[2]) + off[0];
  const double m1 = ((P[3] * p[0] + P[4] * p[1]) + P[5] * p[2]) + off[1];
  const double rad = rn_radius(i00, i10, i11, eps);
  if (!(isfinite(i00) && isfinite(i01) && isfinite(i10) && isfinite(i11) && isfinite(m0) && isfinite(m1) &&
        isfinite(rad)))
    return false;
  mu2[0] = m0; mu2[1] = m1;
  Sinv[0] = i00; Sinv[1] = i01; Sinv[2] = i10; Sinv[3] = i11;
  *r = rad;
  return true;
}

}  // namespace gcs
