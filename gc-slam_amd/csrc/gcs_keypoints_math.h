// Per-pixel math of the keypoint detector (gcs_keypoints.hip), shared by the device kernels and the host
// build of the same steps (gcs_detect_keypoints_host): the grey conversion, the FAST-9/16 segment test
// and score, the 3 x 3 Sobel derivatives, the Harris response and the order-preserving key of a
// response.  Everything is integer arithmetic except the last step of the response, which is f64 with
// every operation rounded on its own and one final rounding to f32.  The pixel readers take a pointer to
// the centre pixel and the distance between rows in bytes, so that the same code reads an LDS tile on the
// device and the whole image on the host.
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

}  // namespace gcs
