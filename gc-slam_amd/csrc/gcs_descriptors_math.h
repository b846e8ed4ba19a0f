// Integer math of the keypoint describer and the descriptor matcher (gcs_descriptors.hip; the definition: D1-D7
// in include/gcslam_hip.h), shared by the device kernels and the host twins: a keypoint's level pixel, the
// direction table and the angle bin, the steering of a pattern point, the pattern itself and the disc of the
// moments.  Everything that decides an output is integer arithmetic; the level pixel is f64 with every operation
// rounded on its own, and the informative angle is the one call of atan2.
#pragma once

#include <math.h>
#include <stdint.h>

#include "gcs_brief_pattern.h"
#include "gcs_math.h"

#pragma clang fp contract(off)

namespace gcs {

constexpr int kKdMargin = 16;          // D1: a keypoint nearer than this to its level's edge is invalid
constexpr int kKdPatch = 2 * kKdMargin + 1;   // 33: the level pixels a keypoint reads, centre included
constexpr int kKdMomentR = 15;         // D2: the disc dx^2 + dy^2 <= 225
constexpr int kKdBoxR = 2;             // D6: the 5 x 5 box
constexpr int kKdBoxes = kKdPatch - 2 * kKdBoxR;   // 29: box centres per row of the patch, offsets -14 .. 14
constexpr int kKdBins = 32;
constexpr int kKdTests = 256, kKdBytes = kKdTests / 8;
constexpr int kKdNoMatch = 257;        // D7: the distance where there is no train row

// D1: floor((double(u) + 0.5) * W_l / W_0), as a double; the caller has checked that u is finite
GCS_HD double kd_level_pixel(float u, int W_l, int W_0) {
  const double a = (double)u + 0.5;
  const double b = a * (double)W_l;
  const double c = b / (double)W_0;
  return floor(c);
}

// D1's last case: the level pixel q (a whole number) lies within the margin of a level W_l wide
GCS_HD bool kd_inside(double q, int W_l) { return q >= (double)kKdMargin && q < (double)W_l - (double)kKdMargin; }

// D3: (C_k, S_k) = 2^14 (cos, sin)(11.25 deg k).  Entries 0..7 are literals, the others follow by quarter turns:
// C_{k+8} = -S_k, S_{k+8} = C_k.
GCS_HD void kd_direction(int k, int* C, int* S) {
  constexpr int16_t c8[8] = {16384, 16069, 15137, 13623, 11585, 9102, 6270, 3196};
  constexpr int16_t s8[8] = {0, 3196, 6270, 9102, 11585, 13623, 15137, 16069};
  int c = c8[k & 7], s = s8[k & 7];
  for (int q = 0; q < (k >> 3); ++q) {
    const int t = c;
    c = -s;
    s = t;
  }
  *C = c;
  *S = s;
}

// D3: the k that maximises m10 C_k + m01 S_k in int64, ties to the lowest k
GCS_HD int kd_angle_bin(int32_t m10, int32_t m01) {
  int best = 0;
  int64_t best_v = 0;
  for (int k = 0; k < kKdBins; ++k) {
    int C, S;
    kd_direction(k, &C, &S);
    const int64_t v = (int64_t)m10 * C + (int64_t)m01 * S;
    if (k == 0 || v > best_v) {
      best = k;
      best_v = v;
    }
  }
  return best;
}

// n / 2^14 rounded half away from zero, in integers
GCS_HD int kd_rnd14(int n) { return n >= 0 ? (n + 8192) >> 14 : -((-n + 8192) >> 14); }

// D5: the pattern point (x, y) steered to the direction (C, S) of a bin
GCS_HD void kd_steer(int x, int y, int C, int S, int* sx, int* sy) {
  *sx = kd_rnd14(x * C - y * S);
  *sy = kd_rnd14(x * S + y * C);
}

// D5: row i of the pattern: ax, ay, bx, by
GCS_HD void kd_pattern(int i, int* p) {
  constexpr int8_t rows[kKdTests][4] = {GCS_BRIEF_PATTERN_ROWS};
  p[0] = rows[i][0];
  p[1] = rows[i][1];
  p[2] = rows[i][2];
  p[3] = rows[i][3];
}

// D2: (dx, dy) lies in the disc of the moments
GCS_HD bool kd_in_disc(int dx, int dy) { return dx * dx + dy * dy <= kKdMomentR * kKdMomentR; }

// D7: the Hamming distance of two 32-byte rows held as 8 words
GCS_HD int kd_hamming(const uint32_t* a, const uint32_t* b) {
  int d = 0;
#pragma unroll
  for (int w = 0; w < 8; ++w) d += __builtin_popcount(a[w] ^ b[w]);
  return d;
}

// D7: one more train row of distance d and index j into a running (dist, idx, dist2); rows come in ascending j,
// so a tie stays with the lower index and counts as the second nearest
GCS_HD void kd_match_step(int d, int j, int* dist, int* idx, int* dist2) {
  if (d < *dist) {
    *dist2 = *dist;
    *dist = d;
    *idx = j;
  } else if (d < *dist2) {
    *dist2 = d;
  }
}

// D8: the levels within max_level_diff of level ql, as int32 bounds: for an int32 level tl, lo <= tl <= hi is
// |tl - ql| <= max_level_diff in exact integers (bounds beyond int32 saturate, which no int32 level can tell apart).
GCS_HD void kd_level_window(int32_t ql, int32_t max_level_diff, int32_t* lo, int32_t* hi) {
  const int64_t a = (int64_t)ql - max_level_diff, b = (int64_t)ql + max_level_diff;
  *lo = (int32_t)(a < INT32_MIN ? INT32_MIN : a);
  *hi = (int32_t)(b > INT32_MAX ? INT32_MAX : b);
}

// D8: position (tu, tv) on level tl lies in the window of radius `radius` around (pu, pv) and of levels lo .. hi.
// Each difference is one float32 subtraction (|a - b| = |b - a| exactly, and so is the level test symmetric, so
// either row may be the query); a NaN or an inf - inf fails its comparison.
GCS_HD bool kd_gate(float tu, float tv, int32_t tl, float pu, float pv, int32_t lo, int32_t hi, float radius) {
  const float du = tu - pu, dv = tv - pv;
  return (int)(fabsf(du) <= radius) & (int)(fabsf(dv) <= radius) & (int)(tl >= lo) & (int)(tl <= hi);
}

// D9: the filters of one query row on its merged (idx, dist, dist2); the cross check is the caller's
GCS_HD bool kd_pair_filters(int idx, int dist, int dist2, int max_distance, int ratio_num, int ratio_den) {
  if (idx < 0 || dist > max_distance) return false;
  return ratio_den == 0 || (int64_t)dist * ratio_den < (int64_t)ratio_num * dist2;
}

}  // namespace gcs
