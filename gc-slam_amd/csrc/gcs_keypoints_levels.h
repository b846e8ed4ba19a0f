// The scale pyramid's packed level table and its resample kernel, shared by the detectors (gcs_keypoints.hip)
// and the describer (gcs_descriptors.hip), so that both see the same bytes of every level's grey image: the
// config checks the table depends on, KpLevels and kp_levels, the table's lookups, kp_resample_pixel and
// k_kpp_resample.  Everything is in an anonymous namespace: each translation unit has its own copy.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include <cmath>

#include "gcs_keypoints_math.h"
#include "gcslam_hip.h"

#pragma clang fp contract(off)

namespace gcs {
namespace {

constexpr int kKpTileW = 64, kKpTileH = 16, kKpThreads = 256;
constexpr int kKpStrip = 2048;

// ---- the pyramid (gcs_detect_keypoints_pyramid)

// The level table of the packed workspace.  The grey and score images of the levels follow one another, each
// level's first pixel on a multiple of 256 (a resample workgroup then has one level); the key image likewise
// with every level on a strip boundary, so a strip has one level.  A level without pixels has no tiles and no
// strips.  [n .. 8] of the three running tables hold the totals.
struct KpLevels {
  int32_t n;
  int32_t W[kKpMaxLevels], H[kKpMaxLevels], quota[kKpMaxLevels], tiles_x[kKpMaxLevels];
  int32_t tile0[kKpMaxLevels + 1], strip0[kKpMaxLevels + 1], block0[kKpMaxLevels + 1];   // block: 256 pixels
};

// the level of tile / strip / block idx: the last one that starts at or before it
__device__ inline int kp_level_at(const int32_t* first, int n, int idx) {
  int l = 0;
#pragma unroll
  for (int m = 1; m < kKpMaxLevels; ++m) l += (m < n && idx >= first[m]);
  return l;
}
// a[l] by selects, so that the table stays in scalar registers
template <int N>
__device__ inline int kp_pick(const int32_t (&a)[N], int l) {
  int v = a[0];
#pragma unroll
  for (int m = 1; m < N; ++m) v = l >= m ? a[m] : v;
  return v;
}

// Pixel (x, y) of the level Wl x Hl wide of a W x H image: the exact pixel-area mean of the grey values under
// it, rounded half up.  Only pixels of [0, W) x [0, H) are read, byte by byte.
template <int CH>
GCS_HD int kp_resample_pixel(const uint8_t* __restrict__ img, int64_t pitch, int W, int H, int Wl, int Hl, int x, int y) {
  const int j0 = kp_src_first(x, W, Wl), j1 = kp_src_last(x, W, Wl);
  const int i0 = kp_src_first(y, H, Hl), i1 = kp_src_last(y, H, Hl);
  int64_t sum = 0;
  for (int i = i0; i <= i1; ++i) {
    const uint8_t* row = img + (int64_t)i * pitch;
    int64_t rs = 0;
    for (int j = j0; j <= j1; ++j) {
      const int g = CH == 3 ? kp_grey(row[3 * (int64_t)j], row[3 * (int64_t)j + 1], row[3 * (int64_t)j + 2]) : row[j];
      rs += kp_overlap(x, j, W, Wl) * g;
    }
    sum += kp_overlap(y, i, H, Hl) * rs;
  }
  const int64_t area = (int64_t)W * H;
  return kp_area_mean(sum, area, kp_area_narrow(area));
}

// every level's grey image from the input, one thread per pixel of the packed image; level 0 is step 1 itself
template <int CH>
__global__ __launch_bounds__(kKpThreads) void k_kpp_resample(const uint8_t* __restrict__ img, int64_t pitch, const KpLevels lv,
                                                             uint8_t* __restrict__ grey_out) {
  const int l = kp_level_at(lv.block0, lv.n, blockIdx.x);
  const int Wl = kp_pick(lv.W, l), Hl = kp_pick(lv.H, l);
  const int local = (blockIdx.x - kp_pick(lv.block0, l)) * kKpThreads + threadIdx.x;
  if (local >= Wl * Hl) return;
  const int x = local % Wl, y = local / Wl;
  int g;
  if (l == 0) {
    const uint8_t* p = img + (int64_t)y * pitch + CH * (int64_t)x;
    g = CH == 3 ? kp_grey(p[0], p[1], p[2]) : p[0];
  } else {
    g = kp_resample_pixel<CH>(img, pitch, lv.W[0], lv.H[0], Wl, Hl, x, y);
  }
  grey_out[(size_t)blockIdx.x * kKpThreads + threadIdx.x] = (uint8_t)g;
}

// ---- checks

inline const char* kp_check_config(const gcs_keypoint_config* c) {
  if (!c) return "null config";
  if (c->fast_threshold < 0 || c->fast_threshold > 255) return "fast_threshold outside [0, 255]";
  if (c->edge_threshold < kKpMinEdge) return "edge_threshold below 4";
  if (c->max_keypoints < 1 || c->max_keypoints > kKpMaxKeypoints) return "max_keypoints outside [1, 65536]";
  if (c->max_width < 1 || c->max_height < 1 || (int64_t)c->max_width * c->max_height > kKpMaxPixels)
    return "max_width or max_height below 1, or more than 2^28 pixels";
  if (!std::isfinite(c->harris_k)) return "harris_k not finite";
  return nullptr;
}

inline const char* kp_check_pyramid_config(const gcs_keypoint_pyramid_config* c) {
  if (!c) return "null config";
  const gcs_keypoint_config six = {c->fast_threshold, c->edge_threshold, c->max_keypoints, c->max_width,
                                   c->max_height, c->harris_k, c->device};
  if (const char* m = kp_check_config(&six)) return m;
  if (c->n_levels < 1 || c->n_levels > kKpMaxLevels) return "n_levels outside [1, 8]";
  if (c->scale_den < 1 || c->scale_num <= c->scale_den || c->scale_num > 2 * c->scale_den || c->scale_num > kKpMaxScaleNum)
    return "scale_num / scale_den outside (1, 2], or scale_num above 64";
  return nullptr;
}

// the level table of a W x H image (W H <= 2^28, so every level's pixel count stays in int32)
inline KpLevels kp_levels(const gcs_keypoint_pyramid_config& c, int W, int H) {
  KpLevels lv{};
  lv.n = c.n_levels;
  kp_quotas(c.max_keypoints, c.n_levels, c.scale_num, c.scale_den, lv.quota);
  for (int l = 0; l < kKpMaxLevels; ++l) {
    int64_t px = 0;
    if (l < lv.n) {
      lv.W[l] = kp_level_size(W, c.scale_num, c.scale_den, l);
      lv.H[l] = kp_level_size(H, c.scale_num, c.scale_den, l);
      if (lv.W[l] >= 1 && lv.H[l] >= 1) px = (int64_t)lv.W[l] * lv.H[l];
    }
    lv.tiles_x[l] = px ? (lv.W[l] + kKpTileW - 1) / kKpTileW : 0;
    lv.tile0[l + 1] = lv.tile0[l] + (px ? lv.tiles_x[l] * ((lv.H[l] + kKpTileH - 1) / kKpTileH) : 0);
    lv.strip0[l + 1] = lv.strip0[l] + (int32_t)((px + kKpStrip - 1) / kKpStrip);
    lv.block0[l + 1] = lv.block0[l] + (int32_t)((px + kKpThreads - 1) / kKpThreads);
  }
  return lv;
}

}  // namespace
}  // namespace gcs
