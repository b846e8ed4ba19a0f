// Keypoint descriptors on the GPU: what ORB adds behind its detector -- the intensity-centroid orientation and a
// steered 256-bit BRIEF descriptor per keypoint -- and a brute-force Hamming matcher.  The project's own
// definition (D1-D7 in include/gcslam_hip.h): the pattern is a fixed pseudo-random one, not ORB's learned rBRIEF
// pattern, and no parity with cv::ORB is claimed.  Every decided output is integer arithmetic
// (gcs_descriptors_math.h), which the host twins run as well.  Kernels:
//   k_kpp_resample  (gcs_keypoints_levels.h) every level's grey image, packed, as the detectors make it
//   k_kp_describe   one wave per keypoint, four keypoints per workgroup: the keypoint's level pixel and validity
//                   (wave-uniform), the 33 x 33 patch into LDS with a 36-byte row pitch (whole dwords per row:
//                   the lanes of a 5-tap pass then touch at most three rows of 9 consecutive dwords, distinct
//                   banks), the horizontal and vertical 5-sums as uint16 (29 x 29 box sums), the moments over
//                   the disc reduced across the 64 lanes, the 32-way integer argmax, then four tests per lane,
//                   packed with __ballot; lanes 0..31 store one byte of the row each.  Invalid rows are
//                   written by the same kernel, so nothing is cleared beforehand.
//   k_match_partial one query row per thread in 8 registers; a workgroup of one wave streams tiles of 128 train
//                   rows through LDS (every lane reads the same address: a broadcast) and keeps (dist, idx,
//                   dist2); the train rows are split over blockIdx.y into up to 32 chunks of at least 128 rows,
//                   whose partial results go to the workspace: 512 x 512 rows are 8 x 4 workgroups
//   k_match_merge   one thread per query row over the chunks: the lexicographic minimum of (dist, idx), and
//                   dist2 = min(the winner's dist2, the other chunks' dist).  With one chunk k_match_partial
//                   writes the outputs itself and this kernel is not launched.

#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "gcs_descriptors_math.h"
#include "gcs_keypoints_levels.h"
#include "gcs_keypoints_math.h"
#include "gcslam_hip.h"

#pragma clang fp contract(off)

namespace gcs {
namespace {

constexpr int kKdWaves = 4, kKdThreads = 64 * kKdWaves;
constexpr int kKdPatchPitch = 36;   // bytes per staged row of 33
constexpr int kKdSumPitch = 30;     // uint16 per row of 29 sums
constexpr int kMtThreads = 64, kMtTile = 128, kMtChunk = 128, kMtMaxSplits = 32;
constexpr int kMtMaxRows = 1 << 20;

__global__ __launch_bounds__(kKdThreads) void k_kp_describe(const uint8_t* __restrict__ grey, const KpLevels lv, int n,
                                                            const float* __restrict__ kp_u, const float* __restrict__ kp_v,
                                                            const int32_t* __restrict__ kp_level,
                                                            gcs_keypoint_desc_outputs o) {
  __shared__ uint8_t patch[kKdWaves][kKdPatch * kKdPatchPitch];
  __shared__ uint16_t hsum[kKdWaves][kKdPatch * kKdSumPitch];
  __shared__ uint16_t box[kKdWaves][kKdBoxes * kKdSumPitch];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * kKdWaves + wave;
  // D1, the same in every lane of the wave
  bool valid = false;
  int x = 0, y = 0, Wl = 0;
  const uint8_t* g = grey;
  if (row < n) {
    const float u = kp_u[row], v = kp_v[row];
    const int l = kp_level ? kp_level[row] : 0;
    if (isfinite(u) && isfinite(v) && l >= 0 && l < lv.n) {
      Wl = kp_pick(lv.W, l);
      const int Hl = kp_pick(lv.H, l);
      if (Wl >= 1 && Hl >= 1) {
        const double qx = kd_level_pixel(u, Wl, lv.W[0]), qy = kd_level_pixel(v, Hl, lv.H[0]);
        if (kd_inside(qx, Wl) && kd_inside(qy, Hl)) {
          valid = true;
          x = (int)qx;
          y = (int)qy;
          g = grey + (size_t)kp_pick(lv.block0, l) * kKpThreads;
        }
      }
    }
  }
  if (valid)   // 16 <= x < Wl - 16 and likewise y: the patch is inside the level
    for (int idx = lane; idx < kKdPatch * kKdPatch; idx += 64) {
      const int r = idx / kKdPatch, c = idx % kKdPatch;
      patch[wave][r * kKdPatchPitch + c] = g[(size_t)(y - kKdMargin + r) * Wl + (x - kKdMargin + c)];
    }
  __syncthreads();
  int m10 = 0, m01 = 0;
  if (valid) {
    for (int idx = lane; idx < kKdPatch * kKdBoxes; idx += 64) {
      const int r = idx / kKdBoxes, c = idx % kKdBoxes;
      const uint8_t* p = &patch[wave][r * kKdPatchPitch + c];
      hsum[wave][r * kKdSumPitch + c] = (uint16_t)(p[0] + p[1] + p[2] + p[3] + p[4]);
    }
    constexpr int side = 2 * kKdMomentR + 1;
    for (int idx = lane; idx < side * side; idx += 64) {
      const int dy = idx / side - kKdMomentR, dx = idx % side - kKdMomentR;
      if (kd_in_disc(dx, dy)) {
        const int v = patch[wave][(kKdMargin + dy) * kKdPatchPitch + kKdMargin + dx];
        m10 += dx * v;
        m01 += dy * v;
      }
    }
  }
  __syncthreads();
  if (valid)
    for (int idx = lane; idx < kKdBoxes * kKdBoxes; idx += 64) {
      const int r = idx / kKdBoxes, c = idx % kKdBoxes;
      const uint16_t* p = &hsum[wave][r * kKdSumPitch + c];
      box[wave][r * kKdSumPitch + c] =
          (uint16_t)(p[0] + p[kKdSumPitch] + p[2 * kKdSumPitch] + p[3 * kKdSumPitch] + p[4 * kKdSumPitch]);
    }
  __syncthreads();
  for (int off = 32; off > 0; off >>= 1) {
    m10 += __shfl_xor(m10, off, 64);
    m01 += __shfl_xor(m01, off, 64);
  }
  int bin = -1;
  unsigned long long words[4] = {0ull, 0ull, 0ull, 0ull};
  if (valid) {
    bin = kd_angle_bin(m10, m01);
    int C, S;
    kd_direction(bin, &C, &S);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int p[4], ax, ay, bx, by;
      kd_pattern(64 * j + lane, p);
      kd_steer(p[0], p[1], C, S, &ax, &ay);
      kd_steer(p[2], p[3], C, S, &bx, &by);
      constexpr int mid = kKdBoxes / 2;   // |steered coordinate| <= 13 < mid = 14
      const int a = box[wave][(mid + ay) * kKdSumPitch + mid + ax], b = box[wave][(mid + by) * kKdSumPitch + mid + bx];
      words[j] = __ballot(a < b);   // bit `lane` of word j is test 64 j + lane: byte i / 8, bit i % 8, little-endian
    }
  }
  if (row >= n) return;
  if (lane < kKdBytes) {
    const unsigned long long w = lane < 8 ? words[0] : lane < 16 ? words[1] : lane < 24 ? words[2] : words[3];
    o.desc[(size_t)row * kKdBytes + lane] = (uint8_t)(w >> (8 * (lane & 7)));
  }
  if (lane == 32) o.kp_angle_bin[row] = bin;
  if (lane == 33) o.kp_angle[row] = valid ? (float)atan2((double)m01, (double)m10) : NAN;
}

// ---- the matcher

// Query rows of blockIdx.x against the train rows [blockIdx.y * chunk, + chunk); the results of chunk c at
// [c * n_q + query] of the three arrays (with one chunk these are the outputs themselves).
__global__ __launch_bounds__(kMtThreads) void k_match_partial(const uint32_t* __restrict__ q, const uint32_t* __restrict__ tr,
                                                              const int32_t* __restrict__ q_bin, const int32_t* __restrict__ t_bin,
                                                              int n_q, int n_t, int chunk, int32_t* __restrict__ idx_out,
                                                              int32_t* __restrict__ dist_out, int32_t* __restrict__ dist2_out) {
  __shared__ uint32_t tile[kMtTile * 8];
  __shared__ int32_t tile_far[kMtTile];   // 0, or on an invalid row what puts its distance beyond every real one
  const int t = threadIdx.x, row = blockIdx.x * kMtThreads + t;
  const bool have = row < n_q;
  uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (have) {
#pragma unroll
    for (int k = 0; k < 8; ++k) w[k] = q[(size_t)row * 8 + k];
  }
  const int j0 = min(n_t, (int)blockIdx.y * chunk), j1 = min(n_t, j0 + chunk);
  int dist = kKdNoMatch, idx = -1, dist2 = kKdNoMatch;
  for (int base = j0; base < j1; base += kMtTile) {
    const int cnt = min(kMtTile, j1 - base);
    __syncthreads();
    for (int i = t; i < cnt * 8; i += kMtThreads) tile[i] = tr[(size_t)base * 8 + i];
    for (int i = t; i < cnt; i += kMtThreads) tile_far[i] = (t_bin && t_bin[base + i] < 0) ? kKdNoMatch : 0;
    __syncthreads();
#pragma unroll 4
    for (int r = 0; r < cnt; ++r)   // (no branch on the row: the loads of the next rows go out under this one's sums)
      kd_match_step(kd_hamming(w, &tile[r * 8]) + tile_far[r], base + r, &dist, &idx, &dist2);
  }
  if (!have) return;
  if (q_bin && q_bin[row] < 0) {
    dist = dist2 = kKdNoMatch;
    idx = -1;
  }
  const size_t at = (size_t)blockIdx.y * n_q + row;
  idx_out[at] = idx;
  dist_out[at] = dist;
  dist2_out[at] = dist2;
}

__global__ __launch_bounds__(kMtThreads) void k_match_merge(const int32_t* __restrict__ p_idx, const int32_t* __restrict__ p_dist,
                                                            const int32_t* __restrict__ p_dist2, int n_q, int n_parts,
                                                            gcs_match_outputs o) {
  const int row = blockIdx.x * kMtThreads + threadIdx.x;
  if (row >= n_q) return;
  int win = 0, dist = p_dist[row];
  for (int c = 1; c < n_parts; ++c) {   // (the chunks are in ascending index order: the first minimum has the lowest index)
    const int d = p_dist[(size_t)c * n_q + row];
    if (d < dist) {
      dist = d;
      win = c;
    }
  }
  int dist2 = p_dist2[(size_t)win * n_q + row];
  for (int c = 0; c < n_parts; ++c)
    if (c != win) dist2 = min(dist2, p_dist[(size_t)c * n_q + row]);
  o.idx[row] = p_idx[(size_t)win * n_q + row];
  o.dist[row] = dist;
  o.dist2[row] = dist2;
}

// ---- checks and the host build

gcs_keypoint_pyramid_config kd_pyramid_config(const gcs_keypoint_desc_config& c) {
  gcs_keypoint_pyramid_config p;
  memset(&p, 0, sizeof(p));
  p.fast_threshold = 20;   // (the detector's fields are not looked at; these pass its checks)
  p.edge_threshold = 31;
  p.harris_k = 0.04;
  p.max_keypoints = c.max_keypoints;
  p.max_width = c.max_width;
  p.max_height = c.max_height;
  p.n_levels = c.n_levels;
  p.scale_num = c.scale_num;
  p.scale_den = c.scale_den;
  p.device = c.device;
  return p;
}

const char* kd_check_config(const gcs_keypoint_desc_config* c) {
  if (!c) return "null config";
  const gcs_keypoint_pyramid_config p = kd_pyramid_config(*c);
  return kp_check_pyramid_config(&p);
}

const char* kd_check_call(const gcs_keypoint_desc_config& c, const gcs_keypoint_inputs* in, const gcs_keypoint_desc_keypoints* k,
                          const gcs_keypoint_desc_outputs* o) {
  if (!in || !k || !o) return "null inputs, keypoints or outputs";
  if (in->channels != 1 && in->channels != 3) return "channels is 1 (gray8) or 3 (rgb8)";
  if (in->width < 1 || in->height < 1 || in->width > c.max_width || in->height > c.max_height)
    return "width or height below 1 or above the context's capacity";
  if (in->pitch < (int64_t)in->channels * in->width) return "pitch below a row";
  if (!in->image) return "null array";
  if (k->n_keypoints < 0 || k->n_keypoints > c.max_keypoints) return "n_keypoints outside [0, max_keypoints]";
  if (k->n_keypoints > 0 && (!k->kp_u || !k->kp_v || !o->kp_angle || !o->kp_angle_bin || !o->desc)) return "null array";
  return nullptr;
}

const char* mt_check_config(const gcs_match_config* c) {
  if (!c) return "null config";
  if (c->max_query < 1 || c->max_query > kMtMaxRows || c->max_train < 1 || c->max_train > kMtMaxRows)
    return "max_query or max_train outside [1, 1048576]";
  return nullptr;
}

const char* mt_check_call(const gcs_match_config& c, const gcs_match_inputs* in, const gcs_match_outputs* o) {
  if (!in || !o) return "null inputs or outputs";
  if (in->n_query < 0 || in->n_query > c.max_query || in->n_train < 0 || in->n_train > c.max_train)
    return "n_query or n_train below 0 or above the context's capacity";
  if (in->n_query > 0 && (!in->q || !o->idx || !o->dist || !o->dist2)) return "null array";
  if (in->n_query > 0 && in->n_train > 0 && !in->t) return "null array";
  if (((uintptr_t)in->q | (uintptr_t)in->t) & 3u) return "q or t not 4-byte aligned";
  return nullptr;
}

// the chunks of n_t train rows: their length (a multiple of the tile) and their number
void mt_split(int n_t, int* chunk, int* n_parts) {
  const int want = std::max(1, std::min(kMtMaxSplits, (n_t + kMtChunk - 1) / kMtChunk));
  const int len = (n_t + want - 1) / want;
  *chunk = std::max(kMtTile, (len + kMtTile - 1) / kMtTile * kMtTile);
  *n_parts = std::max(1, (n_t + *chunk - 1) / *chunk);
}

}  // namespace
}  // namespace gcs

using namespace gcs;

struct gcs_keypoint_desc_ctx {
  gcs_keypoint_desc_config cfg{};
  gcs_keypoint_pyramid_config pyr{};
  std::string err;
  int device = 0;
  hipStream_t stream = nullptr;   // the caller's (gcs_keypoint_desc_ctx_set_stream); null: HIP's default stream
  uint8_t* grey = nullptr;        // the packed grey images of every level
  int cap_blocks = 0;             // in 256-pixel blocks
};

struct gcs_match_ctx {
  gcs_match_config cfg{};
  std::string err;
  int device = 0;
  hipStream_t stream = nullptr;
  int32_t* part = nullptr;        // 3 x kMtMaxSplits x max_query: idx, dist, dist2 of every chunk
};

namespace {
int kd_fail(gcs_keypoint_desc_ctx* c, int code, const std::string& m) {
  if (c) c->err = m;
  return code;
}
int mt_fail(gcs_match_ctx* c, int code, const std::string& m) {
  if (c) c->err = m;
  return code;
}
#define KDCHK(fail, ctx, expr)                                                                     \
  do {                                                                                            \
    hipError_t _e = (expr);                                                                       \
    if (_e != hipSuccess) return fail((ctx), GCS_ERR_HIP, std::string(#expr ": ") + hipGetErrorString(_e)); \
  } while (0)

// the grey value of pixel (x, y) of level l (Wl x Hl) of the input
int kd_host_pixel(const gcs_keypoint_inputs* in, int l, int Wl, int Hl, int x, int y) {
  if (l == 0) {
    const uint8_t* p = in->image + (int64_t)y * in->pitch + (int64_t)in->channels * x;
    return in->channels == 3 ? kp_grey(p[0], p[1], p[2]) : p[0];
  }
  return in->channels == 3 ? kp_resample_pixel<3>(in->image, in->pitch, in->width, in->height, Wl, Hl, x, y)
                           : kp_resample_pixel<1>(in->image, in->pitch, in->width, in->height, Wl, Hl, x, y);
}
}  // namespace

extern "C" {

int gcs_keypoint_desc_config_defaults(gcs_keypoint_desc_config* c) {
  if (!c) return GCS_ERR_ARG;
  gcs_keypoint_pyramid_config ten;
  gcs_keypoint_pyramid_config_defaults(&ten);
  memset(c, 0, sizeof(*c));
  c->n_levels = ten.n_levels;
  c->scale_num = ten.scale_num;
  c->scale_den = ten.scale_den;
  c->max_width = ten.max_width;
  c->max_height = ten.max_height;
  c->max_keypoints = ten.max_keypoints;
  c->device = 0;
  return GCS_OK;
}

int gcs_brief_pattern(int8_t out[256][4]) {
  if (!out) return GCS_ERR_ARG;
  for (int i = 0; i < kKdTests; ++i) {
    int p[4];
    kd_pattern(i, p);
    for (int j = 0; j < 4; ++j) out[i][j] = (int8_t)p[j];
  }
  return GCS_OK;
}

const char* gcs_keypoint_desc_last_error(const gcs_keypoint_desc_ctx* c) {
  return c ? c->err.c_str() : "null keypoint descriptor context";
}

int gcs_keypoint_desc_ctx_destroy(gcs_keypoint_desc_ctx* c) {
  if (!c) return GCS_OK;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  if (c->grey) (void)hipFree(c->grey);
  delete c;
  return GCS_OK;
}

int gcs_keypoint_desc_ctx_create(const gcs_keypoint_desc_config* cfg, gcs_keypoint_desc_ctx** out) {
  if (!cfg || !out) return GCS_ERR_ARG;
  *out = nullptr;
  if (kd_check_config(cfg)) return GCS_ERR_ARG;
  auto* c = new gcs_keypoint_desc_ctx();
  c->cfg = *cfg;
  c->pyr = kd_pyramid_config(*cfg);
  c->device = cfg->device;
  // A level's size grows with the image's, so the table of max_width x max_height bounds every image's.
  c->cap_blocks = kp_levels(c->pyr, cfg->max_width, cfg->max_height).block0[kKpMaxLevels];
  if (hipSetDevice(cfg->device) != hipSuccess ||
      hipMalloc((void**)&c->grey, (size_t)c->cap_blocks * kKpThreads) != hipSuccess) {
    c->grey = nullptr;
    gcs_keypoint_desc_ctx_destroy(c);
    return GCS_ERR_HIP;
  }
  *out = c;
  return GCS_OK;
}

int gcs_keypoint_desc_ctx_set_stream(gcs_keypoint_desc_ctx* c, void* stream) {
  if (!c) return GCS_ERR_ARG;
  hipStream_t ns = (hipStream_t)stream;
  if (ns == c->stream) return GCS_OK;
  KDCHK(kd_fail, c, hipSetDevice(c->device));
  KDCHK(kd_fail, c, hipStreamSynchronize(c->stream));  // the workspace is shared: the old stream's work completes first
  c->stream = ns;
  return GCS_OK;
}

int gcs_describe_keypoints_host(const gcs_keypoint_desc_config* cfg, const gcs_keypoint_inputs* in,
                                const gcs_keypoint_desc_keypoints* kps, gcs_keypoint_desc_outputs* out) {
  if (kd_check_config(cfg) || kd_check_call(*cfg, in, kps, out)) return GCS_ERR_ARG;
  const KpLevels lv = kp_levels(kd_pyramid_config(*cfg), in->width, in->height);
  std::vector<int> patch(kKdPatch * kKdPatch), box(kKdBoxes * kKdBoxes);
  for (int i = 0; i < kps->n_keypoints; ++i) {
    const float u = kps->kp_u[i], v = kps->kp_v[i];
    const int l = kps->kp_level ? kps->kp_level[i] : 0;
    bool valid = false;
    int x = 0, y = 0, Wl = 0, Hl = 0;
    if (std::isfinite(u) && std::isfinite(v) && l >= 0 && l < lv.n) {
      Wl = lv.W[l];
      Hl = lv.H[l];
      if (Wl >= 1 && Hl >= 1) {
        const double qx = kd_level_pixel(u, Wl, lv.W[0]), qy = kd_level_pixel(v, Hl, lv.H[0]);
        if (kd_inside(qx, Wl) && kd_inside(qy, Hl)) {
          valid = true;
          x = (int)qx;
          y = (int)qy;
        }
      }
    }
    uint8_t* row = out->desc + (size_t)i * kKdBytes;
    memset(row, 0, kKdBytes);
    if (!valid) {
      out->kp_angle[i] = NAN;
      out->kp_angle_bin[i] = -1;
      continue;
    }
    for (int r = 0; r < kKdPatch; ++r)
      for (int c = 0; c < kKdPatch; ++c) patch[r * kKdPatch + c] = kd_host_pixel(in, l, Wl, Hl, x - kKdMargin + c, y - kKdMargin + r);
    int32_t m10 = 0, m01 = 0;
    for (int dy = -kKdMomentR; dy <= kKdMomentR; ++dy)
      for (int dx = -kKdMomentR; dx <= kKdMomentR; ++dx)
        if (kd_in_disc(dx, dy)) {
          const int g = patch[(kKdMargin + dy) * kKdPatch + kKdMargin + dx];
          m10 += dx * g;
          m01 += dy * g;
        }
    for (int r = 0; r < kKdBoxes; ++r)
      for (int c = 0; c < kKdBoxes; ++c) {
        int s = 0;
        for (int a = 0; a <= 2 * kKdBoxR; ++a)
          for (int b = 0; b <= 2 * kKdBoxR; ++b) s += patch[(r + a) * kKdPatch + c + b];
        box[r * kKdBoxes + c] = s;
      }
    const int bin = kd_angle_bin(m10, m01);
    int C, S;
    kd_direction(bin, &C, &S);
    constexpr int mid = kKdBoxes / 2;
    for (int t = 0; t < kKdTests; ++t) {
      int p[4], ax, ay, bx, by;
      kd_pattern(t, p);
      kd_steer(p[0], p[1], C, S, &ax, &ay);
      kd_steer(p[2], p[3], C, S, &bx, &by);
      if (box[(mid + ay) * kKdBoxes + mid + ax] < box[(mid + by) * kKdBoxes + mid + bx]) row[t / 8] |= (uint8_t)(1u << (t % 8));
    }
    out->kp_angle_bin[i] = bin;
    out->kp_angle[i] = (float)atan2((double)m01, (double)m10);
  }
  return GCS_OK;
}

int gcs_describe_keypoints(gcs_keypoint_desc_ctx* c, const gcs_keypoint_inputs* in, const gcs_keypoint_desc_keypoints* kps,
                           gcs_keypoint_desc_outputs* out) {
  if (!c) return GCS_ERR_ARG;
  if (const char* m = kd_check_call(c->cfg, in, kps, out)) return kd_fail(c, GCS_ERR_ARG, m);
  const KpLevels lv = kp_levels(c->pyr, in->width, in->height);
  const int n_blocks = lv.block0[kKpMaxLevels], n = kps->n_keypoints;
  if (n_blocks > c->cap_blocks) return kd_fail(c, GCS_ERR_ARG, "the image's levels exceed the workspace");
  if (n == 0) return GCS_OK;
  KDCHK(kd_fail, c, hipSetDevice(c->device));
  if (in->channels == 3)
    hipLaunchKernelGGL(k_kpp_resample<3>, dim3(n_blocks), dim3(kKpThreads), 0, c->stream, in->image, in->pitch, lv, c->grey);
  else
    hipLaunchKernelGGL(k_kpp_resample<1>, dim3(n_blocks), dim3(kKpThreads), 0, c->stream, in->image, in->pitch, lv, c->grey);
  hipLaunchKernelGGL(k_kp_describe, dim3((n + kKdWaves - 1) / kKdWaves), dim3(kKdThreads), 0, c->stream, c->grey, lv, n,
                     kps->kp_u, kps->kp_v, kps->kp_level, *out);
  KDCHK(kd_fail, c, hipGetLastError());
  return GCS_OK;
}

// ---- the matcher

int gcs_match_config_defaults(gcs_match_config* c) {
  if (!c) return GCS_ERR_ARG;
  memset(c, 0, sizeof(*c));
  c->max_query = 4096;
  c->max_train = 4096;
  c->device = 0;
  return GCS_OK;
}

const char* gcs_match_last_error(const gcs_match_ctx* c) { return c ? c->err.c_str() : "null match context"; }

int gcs_match_ctx_destroy(gcs_match_ctx* c) {
  if (!c) return GCS_OK;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  if (c->part) (void)hipFree(c->part);
  delete c;
  return GCS_OK;
}

int gcs_match_ctx_create(const gcs_match_config* cfg, gcs_match_ctx** out) {
  if (!cfg || !out) return GCS_ERR_ARG;
  *out = nullptr;
  if (mt_check_config(cfg)) return GCS_ERR_ARG;
  auto* c = new gcs_match_ctx();
  c->cfg = *cfg;
  c->device = cfg->device;
  // (mt_split gives n_train rows at most min(kMtMaxSplits, ceil(n_train / kMtChunk)) chunks, which grows with n_train)
  const int parts = std::max(1, std::min(kMtMaxSplits, (cfg->max_train + kMtChunk - 1) / kMtChunk));
  if (hipSetDevice(cfg->device) != hipSuccess ||
      hipMalloc((void**)&c->part, sizeof(int32_t) * 3 * (size_t)parts * (size_t)cfg->max_query) != hipSuccess) {
    c->part = nullptr;
    gcs_match_ctx_destroy(c);
    return GCS_ERR_HIP;
  }
  *out = c;
  return GCS_OK;
}

int gcs_match_ctx_set_stream(gcs_match_ctx* c, void* stream) {
  if (!c) return GCS_ERR_ARG;
  hipStream_t ns = (hipStream_t)stream;
  if (ns == c->stream) return GCS_OK;
  KDCHK(mt_fail, c, hipSetDevice(c->device));
  KDCHK(mt_fail, c, hipStreamSynchronize(c->stream));  // the workspace is shared: the old stream's work completes first
  c->stream = ns;
  return GCS_OK;
}

int gcs_match_descriptors_host(const gcs_match_config* cfg, const gcs_match_inputs* in, gcs_match_outputs* out) {
  if (mt_check_config(cfg) || mt_check_call(*cfg, in, out)) return GCS_ERR_ARG;
  for (int i = 0; i < in->n_query; ++i) {
    int dist = kKdNoMatch, idx = -1, dist2 = kKdNoMatch;
    if (!in->q_bin || in->q_bin[i] >= 0) {
      uint32_t a[8], b[8];
      memcpy(a, in->q + (size_t)i * kKdBytes, kKdBytes);
      for (int j = 0; j < in->n_train; ++j) {
        if (in->t_bin && in->t_bin[j] < 0) continue;
        memcpy(b, in->t + (size_t)j * kKdBytes, kKdBytes);
        kd_match_step(kd_hamming(a, b), j, &dist, &idx, &dist2);
      }
    }
    out->idx[i] = idx;
    out->dist[i] = dist;
    out->dist2[i] = dist2;
  }
  return GCS_OK;
}

int gcs_match_descriptors(gcs_match_ctx* c, const gcs_match_inputs* in, gcs_match_outputs* out) {
  if (!c) return GCS_ERR_ARG;
  if (const char* m = mt_check_call(c->cfg, in, out)) return mt_fail(c, GCS_ERR_ARG, m);
  const int n_q = in->n_query, n_t = in->n_train;
  if (n_q == 0) return GCS_OK;
  int chunk, parts;
  mt_split(n_t, &chunk, &parts);
  KDCHK(mt_fail, c, hipSetDevice(c->device));
  const int q_blocks = (n_q + kMtThreads - 1) / kMtThreads;
  const size_t plane = (size_t)parts * (size_t)n_q;   // three of them fit the workspace (gcs_match_ctx_create)
  int32_t *p_idx = c->part, *p_dist = c->part + plane, *p_dist2 = c->part + 2 * plane;
  if (parts == 1) {
    p_idx = out->idx;
    p_dist = out->dist;
    p_dist2 = out->dist2;
  }
  hipLaunchKernelGGL(k_match_partial, dim3(q_blocks, parts), dim3(kMtThreads), 0, c->stream, (const uint32_t*)in->q,
                     (const uint32_t*)in->t, in->q_bin, in->t_bin, n_q, n_t, chunk, p_idx, p_dist, p_dist2);
  if (parts > 1)
    hipLaunchKernelGGL(k_match_merge, dim3(q_blocks), dim3(kMtThreads), 0, c->stream, p_idx, p_dist, p_dist2, n_q, parts, *out);
  KDCHK(mt_fail, c, hipGetLastError());
  return GCS_OK;
}

}  // extern "C"
