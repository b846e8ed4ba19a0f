// Per-pixel math of the keypoint detector (gcs_keypoints.hip), shared by the device kernels and the host
// build of the same steps (gcs_detect_keypoints_host): the grey conversion, the FAST-9/16 segment test
// and score, the 3 x 3 Sobel derivatives, the Harris response and the order-preserving key of a
// response.  Everything is integer arithmetic except the last step of the response, which is f64 with
// every operation rounded on its own and one final rounding to f32.  The pixel readers take a pointer to
// the centre pixel and the distance between rows in bytes, so that the same code reads an LDS tile on the
// device and the whole image on the host.
// Below them the scale pyramid's integer arithmetic (gcs_detect_keypoints_pyramid): level sizes, the area
// resample's overlap weights, the quotas and the map back to level-0 coordinates.
#pragma once

#include <stdint.h>

#include "gcs_math.h"
#include "gcslam_hip.h"

#pragma clang fp contract(off)

namespace gcs {

constexpr int kKpRing = 16;
constexpr int kKpArc = 9;
constexpr int kKpFrame = 3;        // radius of the ring: the score is 0 nearer than this to the image's edge
constexpr int kKpMinEdge = 4;      // smallest edge_threshold: the 7 x 7 block and its Sobel taps stay inside
constexpr int kKpBlock = 7;        // side of the Harris block
constexpr int kKpMaxKeypoints = 1 << 16;
constexpr int64_t kKpMaxPixels = (int64_t)1 << 28;   // pixel indices and counts stay in int32

// g = (4899 R + 9617 G + 1868 B + 8192) >> 14: the weights sum to 16384, so g <= 255
GCS_HD int kp_grey(int r, int g, int b) { return (4899 * r + 9617 * g + 1868 * b + 8192) >> 14; }

// the radius-3 Bresenham circle, clockwise from the top
GCS_HD int kp_ring_dx(int j) {
  constexpr int8_t dx[kKpRing] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
  return dx[j];
}
GCS_HD int kp_ring_dy(int j) {
  constexpr int8_t dy[kKpRing] = {-3, -3, -2, -1, 0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3};
  return dy[j];
}

// a 16-bit ring mask holds a run of 9 set bits (cyclically) exactly when this is non-zero
GCS_HD uint32_t kp_has_arc(uint32_t mask16) {
  const uint32_t m = mask16 | (mask16 << 16);
  uint32_t r = m & (m >> 1);      // runs of 2
  r &= r >> 2;                    // 4
  r &= r >> 4;                    // 8
  r &= m >> 8;                    // 9
  return r & 0xffffu;
}

// The FAST-9/16 score of the pixel at c (rows `stride` bytes apart; the ring must be readable): m(p) =
// max over the 16 arcs of 9 consecutive ring positions of max(min d_j, min -d_j) when that exceeds
// `threshold`, else 0.  m > threshold exactly when 9 consecutive d_j > threshold or 9 consecutive
// -d_j > threshold, which the two masks decide; only then are the arcs' minima taken.
GCS_HD int kp_fast_score(const uint8_t* c, int64_t stride, int threshold) {
  const int p = c[0];
  int d[kKpRing];
  uint32_t bright = 0, dark = 0;
#pragma unroll
  for (int j = 0; j < kKpRing; ++j) {
    d[j] = (int)c[(int64_t)kp_ring_dy(j) * stride + kp_ring_dx(j)] - p;
    bright |= (uint32_t)(d[j] > threshold) << j;
    dark |= (uint32_t)(-d[j] > threshold) << j;
  }
  if (!(kp_has_arc(bright) | kp_has_arc(dark))) return 0;
  // the minimum and maximum over the runs of 2, 4 and 8 positions that start at each s, then of 9
  int lo[kKpRing], hi[kKpRing];
#pragma unroll
  for (int s = 0; s < kKpRing; ++s) lo[s] = hi[s] = d[s];
#pragma unroll
  for (int w = 1; w < 8; w *= 2) {
    int l2[kKpRing], h2[kKpRing];
#pragma unroll
    for (int s = 0; s < kKpRing; ++s) {
      const int o = (s + w) & (kKpRing - 1);
      l2[s] = lo[o] < lo[s] ? lo[o] : lo[s];
      h2[s] = hi[o] > hi[s] ? hi[o] : hi[s];
    }
#pragma unroll
    for (int s = 0; s < kKpRing; ++s) { lo[s] = l2[s]; hi[s] = h2[s]; }
  }
  int m = 0;
#pragma unroll
  for (int s = 0; s < kKpRing; ++s) {
    const int v = d[(s + 8) & (kKpRing - 1)];
    const int l = v < lo[s] ? v : lo[s], h = v > hi[s] ? v : hi[s];
    const int a = l > -h ? l : -h;   // max(min d, min -d) over the arc that starts at s
    m = a > m ? a : m;
  }
  return m > threshold ? m : 0;
}

// 3 x 3 Sobel derivatives of the grey image at c
GCS_HD void kp_sobel(const uint8_t* c, int64_t stride, int* ix, int* iy) {
  const int a = c[-stride - 1], b = c[-stride], d = c[-stride + 1];
  const int e = c[-1], f = c[1];
  const int g = c[stride - 1], h = c[stride], i = c[stride + 1];
  *ix = (d + 2 * f + i) - (a + 2 * e + g);
  *iy = (g + 2 * h + i) - (a + 2 * b + d);
}

// r = ((double)(a b - c c) - harris_k (double)((a + b)(a + b))) s^4, s = 1 / (4 * 7 * 255), as float32
GCS_HD float kp_response(int64_t a, int64_t b, int64_t c, double harris_k) {
  const double s = 1.0 / (4.0 * (double)kKpBlock * 255.0);
  const double s4 = ((s * s) * s) * s;
  const double det = (double)(a * b - c * c);
  const double tr2 = (double)((a + b) * (a + b));
  const double kt = harris_k * tr2;
  const double r = (det - kt) * s4;
  return (float)r;
}

// the order-preserving map of a float32's bits to uint32; 0 is no finite float's key
GCS_HD uint32_t kp_key_of_bits(uint32_t b) { return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
GCS_HD uint32_t kp_bits_of_key(uint32_t k) { return (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k; }

// ---- the scale pyramid (gcs_detect_keypoints_pyramid): level sizes, area weights, quotas, the coordinate map

constexpr int kKpMaxLevels = 8;
constexpr int kKpMaxScaleNum = 64;

// b^l for 1 <= b <= 64, 0 <= l <= 7: below 2^43
GCS_HD int64_t kp_ipow(int b, int l) {
  int64_t r = 1;
  for (int i = 0; i < l; ++i) r *= b;
  return r;
}

// W_l = (2 W D + N) / (2 N), N = scale_num^l, D = scale_den^l: W D / N rounded half up.  W D can pass 2^63 at
// the largest widths and denominators, so the quotient is formed in 128 bits.
GCS_HD int kp_level_size(int W, int scale_num, int scale_den, int l) {
  const unsigned __int128 N = (unsigned __int128)kp_ipow(scale_num, l), D = (unsigned __int128)kp_ipow(scale_den, l);
  return (int)((2 * (unsigned __int128)W * D + N) / (2 * N));
}

// In units of 1 / W_l of a source pixel, destination pixel x covers [x W, (x + 1) W) and source pixel j covers
// [j W_l, (j + 1) W_l): the integer length of their overlap.  Over j it sums to W.
GCS_HD int64_t kp_overlap(int x, int j, int W, int W_l) {
  const int64_t a0 = (int64_t)x * W, a1 = a0 + W, b0 = (int64_t)j * W_l, b1 = b0 + W_l;
  const int64_t lo = a0 > b0 ? a0 : b0, hi = a1 < b1 ? a1 : b1;
  return hi > lo ? hi - lo : 0;
}
// the first and the last source pixel that destination pixel x overlaps
GCS_HD int kp_src_first(int x, int W, int W_l) { return (int)(((int64_t)x * W) / W_l); }
GCS_HD int kp_src_last(int x, int W, int W_l) { return (int)((((int64_t)x + 1) * W - 1) / W_l); }

// I_l = (sum + (W H) / 2) / (W H) of the weighted sum over the footprint; `narrow`: sum + W H / 2 < 2^32
GCS_HD int kp_area_mean(int64_t sum, int64_t area, bool narrow) {
  if (narrow) return (int)((uint32_t)(sum + area / 2) / (uint32_t)area);
  return (int)((uint64_t)(sum + area / 2) / (uint64_t)area);
}
GCS_HD bool kp_area_narrow(int64_t area) { return area <= (int64_t)0xffffffffu / 256; }

// quota_l: K w_l / sum w (integer division) with w_l = scale_den^l scale_num^(L - 1 - l) for l >= 1; level 0
// takes what is left of K
GCS_HD void kp_quotas(int K, int L, int scale_num, int scale_den, int32_t* quota) {
  int64_t w[kKpMaxLevels], sum = 0;
  for (int l = 0; l < L; ++l) sum += w[l] = kp_ipow(scale_den, l) * kp_ipow(scale_num, L - 1 - l);
  int rest = K;
  for (int l = 1; l < L; ++l) rest -= quota[l] = (int32_t)(((int64_t)K * w[l]) / sum);
  quota[0] = rest;
  for (int l = L; l < kKpMaxLevels; ++l) quota[l] = 0;
}

// the level-0 coordinate of the centre of pixel x of a level W_l wide: (2 x + 1) W / (2 W_l) - 0.5; the
// integers are exact, the division and the subtraction are rounded on their own, then once to float32
GCS_HD float kp_level0_coord(int x, int W, int W_l) {
  const double q = (double)((2 * (int64_t)x + 1) * W) / (double)(2 * (int64_t)W_l);
  return (float)(q - 0.5);
}

// ---- the grid of cells (gcs_detect_keypoints_grid): cell counts, budgets, the cap

constexpr int kKgMinCell = 8, kKgMaxCell = 64;
constexpr int kKgMaxPerCell = 1024;   // strict 3 x 3 suppression: at most ceil(64 / 2)^2 survivors in a cell

// n_cx of a level W_l wide: the cells that cover [e, W_l - e), the last one maybe partial; 0 without such pixels
GCS_HD int kg_cells(int W_l, int edge, int cell_size) {
  const int64_t kept = (int64_t)W_l - 2 * (int64_t)edge;
  return kept > 0 ? (int)((kept + cell_size - 1) / cell_size) : 0;
}

// b_l = min(quota_l, s_l); with `redistribute` what the levels leave of their quotas goes to the levels that
// have survivors beyond theirs, the finest first
GCS_HD void kg_budgets(const int32_t* quota, const int32_t* surv, int redistribute, int32_t* b) {
  int64_t spare = 0;
  for (int l = 0; l < kKpMaxLevels; ++l) {
    b[l] = quota[l] < surv[l] ? quota[l] : surv[l];
    spare += quota[l] - b[l];
  }
  if (!redistribute) return;
  for (int l = 0; l < kKpMaxLevels; ++l) {
    const int64_t room = surv[l] - b[l], give = spare < room ? spare : room;
    b[l] += (int32_t)give;
    spare -= give;
  }
}

// The cap t of a level from cells_with[n - 1], the number of its cells that hold exactly n survivors
// (1 <= n <= 1024): the largest t with sum_c min(n_c, t) <= b, no larger than max_c n_c; *kept_at_t: that sum.
inline int kg_cap_host(const int32_t* cells_with, int64_t b, int64_t* kept_at_t) {
  int t = 0;
  int64_t sum = 0;
  for (;;) {
    int64_t deeper = 0;   // the cells with more than t survivors
    for (int n = t + 1; n <= kKgMaxPerCell; ++n) deeper += cells_with[n - 1];
    if (deeper == 0 || sum + deeper > b) break;
    sum += deeper;
    ++t;
  }
  *kept_at_t = sum;
  return t;
}

}  // namespace gcs
