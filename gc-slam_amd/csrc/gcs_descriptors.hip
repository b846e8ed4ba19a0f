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
//   k_match_gated_partial, k_match_gated_merge   the same two with D8's gate (the tile carries u, v, level and
//                   validity of its rows in one 16-byte entry; the gate is an added distance) and the candidate
//                   counts; blockIdx.z is the direction, so the forward and backward searches of
//                   gcs_match_pairs are one launch and their merges another
//   k_pairs_count, k_pairs_write   D9: the keep flags from the merged results, the kept rows of every 256 (only
//                   where there is more than one such block), then the stable compaction by ballots and sums,
//                   the tails and the count

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

// ---- the gated matcher and the pairs (D8, D9)

// One direction of a gated search: `q` are the rows a thread holds, `t` the rows that stream through the tiles.
// Forward, q is the query set with its prediction and t the train set; backward the two change places (D8's C is
// symmetric in how it is evaluated: |a - b| = |b - a|).
struct MtSearch {
  const uint32_t *q, *t;
  const int32_t *q_bin, *t_bin;
  const float *q_u, *q_v, *t_u, *t_v;   // used with a gate only
  const int32_t *q_level, *t_level;     // null: level 0
  int n_q, n_t, chunk, parts;
  int32_t* part;                        // 4 planes of parts x n_q: idx, dist, dist2, n_cand of every chunk
  int32_t *idx, *dist, *dist2, *n_cand; // the merged results; all but idx may be null
};
struct MtSearches {
  MtSearch s[2];
  float radius;
  int max_level_diff;
};

// k_match_partial with D8's gate: the tile carries (u, v, level, far) of its rows in one 16-byte entry beside the
// descriptors, the gate is a distance of 257 added to the row's like tile_far, and the candidates are counted per
// chunk.  blockIdx.z is the direction; a workgroup outside its direction's extent leaves at once.
template <bool kGate>
__global__ __launch_bounds__(kMtThreads) void k_match_gated_partial(const MtSearches p) {
  __shared__ uint32_t tile[kMtTile * 8];
  __shared__ int4 tile_g[kMtTile];   // with a gate u and v as bits (u NaN on an invalid row) and level; without, .w = 0 or 257
  const MtSearch s = blockIdx.z == 0 ? p.s[0] : p.s[1];
  if ((int)blockIdx.x * kMtThreads >= s.n_q || (int)blockIdx.y >= s.parts) return;
  const int t = threadIdx.x, row = blockIdx.x * kMtThreads + t;
  const bool have = row < s.n_q;
  uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  float pu = NAN, pv = NAN;
  int lo = 0, hi = 0;
  if (have) {
#pragma unroll
    for (int k = 0; k < 8; ++k) w[k] = s.q[(size_t)row * 8 + k];
    if (kGate) {
      pu = s.q_u[row];
      pv = s.q_v[row];
      kd_level_window(s.q_level ? s.q_level[row] : 0, p.max_level_diff, &lo, &hi);
    }
  }
  const int j0 = min(s.n_t, (int)blockIdx.y * s.chunk), j1 = min(s.n_t, j0 + s.chunk);
  int dist = kKdNoMatch, idx = -1, dist2 = kKdNoMatch, n_cand = 0;
  for (int base = j0; base < j1; base += kMtTile) {
    const int cnt = min(kMtTile, j1 - base);
    __syncthreads();
    for (int i = t; i < cnt * 8; i += kMtThreads) tile[i] = s.t[(size_t)base * 8 + i];
    for (int i = t; i < cnt; i += kMtThreads) {
      const bool valid = !(s.t_bin && s.t_bin[base + i] < 0);
      int4 g = make_int4(0, 0, 0, valid ? 0 : kKdNoMatch);
      if (kGate) {   // (an invalid row fails the gate by its NaN: one test less per row and thread)
        g.x = __float_as_int(valid ? s.t_u[base + i] : NAN);
        g.y = __float_as_int(s.t_v[base + i]);
        g.z = s.t_level ? s.t_level[base + i] : 0;
      }
      tile_g[i] = g;
    }
    __syncthreads();
#pragma unroll 4
    for (int r = 0; r < cnt; ++r) {   // (no branch on the row, as in k_match_partial: the gate is a select)
      const int4 g = tile_g[r];
      const bool ok = kGate ? kd_gate(__int_as_float(g.x), __int_as_float(g.y), g.z, pu, pv, lo, hi, p.radius) : g.w == 0;
      n_cand += ok;
      kd_match_step(kd_hamming(w, &tile[r * 8]) + (ok ? 0 : kKdNoMatch), base + r, &dist, &idx, &dist2);
    }
  }
  if (!have) return;
  if (s.q_bin && s.q_bin[row] < 0) {
    dist = dist2 = kKdNoMatch;
    idx = -1;
    n_cand = 0;
  }
  const size_t plane = (size_t)s.parts * s.n_q, at = (size_t)blockIdx.y * s.n_q + row;
  s.part[at] = idx;
  s.part[plane + at] = dist;
  s.part[2 * plane + at] = dist2;
  s.part[3 * plane + at] = n_cand;
}

// k_match_merge for both directions (blockIdx.z), with the chunks' candidate counts added up.
__global__ __launch_bounds__(kMtThreads) void k_match_gated_merge(const MtSearches p) {
  const MtSearch s = blockIdx.z == 0 ? p.s[0] : p.s[1];
  const int row = blockIdx.x * kMtThreads + threadIdx.x;
  if (row >= s.n_q) return;
  const size_t plane = (size_t)s.parts * s.n_q;
  const int32_t *p_idx = s.part, *p_dist = s.part + plane, *p_dist2 = s.part + 2 * plane, *p_cand = s.part + 3 * plane;
  int win = 0, dist = p_dist[row], n_cand = p_cand[row];
  for (int c = 1; c < s.parts; ++c) {   // (the chunks are in ascending index order: the first minimum has the lowest index)
    const int d = p_dist[(size_t)c * s.n_q + row];
    n_cand += p_cand[(size_t)c * s.n_q + row];
    if (d < dist) {
      dist = d;
      win = c;
    }
  }
  int dist2 = p_dist2[(size_t)win * s.n_q + row];
  for (int c = 0; c < s.parts; ++c)
    if (c != win) dist2 = min(dist2, p_dist[(size_t)c * s.n_q + row]);
  s.idx[row] = p_idx[(size_t)win * s.n_q + row];
  if (s.dist) s.dist[row] = dist;
  if (s.dist2) s.dist2[row] = dist2;
  if (s.n_cand) s.n_cand[row] = n_cand;
}

constexpr int kPcThreads = 256;   // the rows one compaction workgroup covers: one per thread
constexpr int kPcWaves = kPcThreads / 64;

struct MtPairs {
  const int32_t *idx, *dist, *dist2;   // the merged forward search
  const int32_t* back;                 // the merged backward idx, one per train row (cross_check)
  int n_q, n_blocks;
  gcs_match_filter f;
  int32_t* block_count;                // n_blocks, written by k_pairs_count (n_blocks > 1)
  gcs_match_pair_outputs o;
};

// D9: query row `row` is kept
__device__ __forceinline__ bool pc_keep(const MtPairs& p, int row) {
  if (row >= p.n_q) return false;
  const int i = p.idx[row];
  if (!kd_pair_filters(i, p.dist[row], p.dist2[row], p.f.max_distance, p.f.ratio_num, p.f.ratio_den)) return false;
  return !p.f.cross_check || p.back[i] == row;
}

// the workgroup's sum of v (every thread gets it); `red` holds one entry per wave
__device__ __forceinline__ int pc_block_sum(int v, int* red) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  int s = 0;
#pragma unroll
  for (int k = 0; k < kPcWaves; ++k) s += red[k];
  return s;
}

// The kept rows of every 256: launched only where there is more than one such block.
__global__ __launch_bounds__(kPcThreads) void k_pairs_count(const MtPairs p) {
  __shared__ int red[kPcWaves];
  const int n = pc_block_sum(pc_keep(p, blockIdx.x * kPcThreads + threadIdx.x) ? 1 : 0, red);
  if (threadIdx.x == 0) p.block_count[blockIdx.x] = n;
}

// The stable compaction: a kept row goes to (kept rows of the blocks before) + (kept rows before it in its block),
// by ballots and sums, so the order is the rows' own and nothing depends on timing.  Row r >= count writes the
// tail entry r itself; the kept rows land below the count, so the two never meet.
__global__ __launch_bounds__(kPcThreads) void k_pairs_write(const MtPairs p) {
  __shared__ int red[kPcWaves], wave_n[kPcWaves];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, row = blockIdx.x * kPcThreads + t;
  const bool keep = pc_keep(p, row);
  const unsigned long long mask = __ballot(keep);
  if (lane == 0) wave_n[wave] = __popcll(mask);
  int before = 0, all = 0;
  if (p.n_blocks > 1) {
    for (int k = t; k < p.n_blocks; k += kPcThreads) {
      const int c = p.block_count[k];
      all += c;
      before += k < (int)blockIdx.x ? c : 0;
    }
    before = pc_block_sum(before, red);
    all = pc_block_sum(all, red);   // (its barriers also publish wave_n)
  } else {
    __syncthreads();
    for (int k = 0; k < kPcWaves; ++k) all += wave_n[k];
  }
  int at = before + __popcll(mask & ((1ull << lane) - 1ull));
  for (int k = 0; k < wave; ++k) at += wave_n[k];
  if (keep) {
    p.o.pair_a[at] = row;
    p.o.pair_b[at] = p.idx[row];
    p.o.pair_dist[at] = p.dist[row];
  }
  if (row < p.n_q && row >= all) {
    p.o.pair_a[row] = -1;
    p.o.pair_b[row] = -1;
    p.o.pair_dist[row] = kKdNoMatch;
  }
  if (row == 0) *p.o.count = all;
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

// the most chunks mt_split gives any n_t up to max_t (their number grows with n_t)
int mt_max_parts(int max_t) { return std::max(1, std::min(kMtMaxSplits, (max_t + kMtChunk - 1) / kMtChunk)); }

const char* mt_check_gate(const gcs_match_inputs* in, const gcs_match_gate* g) {
  if (!std::isfinite(g->radius) || g->radius < 0.0f) return "radius is NaN, infinite or negative";
  if (g->max_level_diff < 0) return "max_level_diff below 0";
  if (!g->q_pu != !g->q_pv) return "q_pu without q_pv, or the reverse";
  if (in->n_query > 0 && !g->q_pu && (!g->q_u || !g->q_v)) return "null position array";
  if (in->n_query > 0 && in->n_train > 0 && (!g->t_u || !g->t_v)) return "null position array";
  return nullptr;
}

const char* mt_check_gated(const gcs_match_config& c, const gcs_match_inputs* in, const gcs_match_gate* g,
                           const gcs_match_gated_outputs* o) {
  if (!in || !g || !o) return "null inputs, gate or outputs";
  const gcs_match_outputs three = {o->idx, o->dist, o->dist2};
  if (const char* m = mt_check_call(c, in, &three)) return m;
  return mt_check_gate(in, g);
}

const char* mt_check_pairs(const gcs_match_config& c, const gcs_match_inputs* in, const gcs_match_gate* g,
                           const gcs_match_filter* f, const gcs_match_pair_outputs* o) {
  if (!in || !f || !o) return "null inputs, filter or outputs";
  if (!o->count) return "null array";
  const gcs_match_outputs three = {o->pair_a, o->pair_b, o->pair_dist};
  if (const char* m = mt_check_call(c, in, &three)) return m;
  if (f->ratio_num < 1 || f->ratio_num > (1 << 20) || f->ratio_den < 0 || f->ratio_den > (1 << 20))
    return "ratio_num outside [1, 1048576] or ratio_den outside [0, 1048576]";
  return g ? mt_check_gate(in, g) : nullptr;
}

// D8's C(i, j) on the host; a null gate: both rows valid
bool mt_host_candidate(const gcs_match_inputs* in, const gcs_match_gate* g, int i, int j) {
  if ((in->q_bin && in->q_bin[i] < 0) || (in->t_bin && in->t_bin[j] < 0)) return false;
  if (!g) return true;
  const float pu = g->q_pu ? g->q_pu[i] : g->q_u[i], pv = g->q_pv ? g->q_pv[i] : g->q_v[i];
  int32_t lo, hi;
  kd_level_window(g->q_level ? g->q_level[i] : 0, g->max_level_diff, &lo, &hi);
  return kd_gate(g->t_u[j], g->t_v[j], g->t_level ? g->t_level[j] : 0, pu, pv, lo, hi, g->radius);
}

int mt_host_distance(const gcs_match_inputs* in, int i, int j) {
  uint32_t a[8], b[8];
  memcpy(a, in->q + (size_t)i * kKdBytes, kKdBytes);
  memcpy(b, in->t + (size_t)j * kKdBytes, kKdBytes);
  return kd_hamming(a, b);
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
  // One allocation.  part: 4 planes (idx, dist, dist2, n_cand; gcs_match_descriptors uses three) of every chunk of
  // max_train for max_query rows; then, for gcs_match_pairs, the same of the backward direction (the chunks of
  // max_query for max_train rows), the merged forward search (3 x max_query), the merged backward idx (max_train)
  // and the kept rows of every 256 query rows.
  int32_t* part = nullptr;
  int32_t *part_back = nullptr, *merged = nullptr, *merged_back = nullptr, *block_count = nullptr;
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
  const size_t n_part = 4 * (size_t)mt_max_parts(cfg->max_train) * (size_t)cfg->max_query;
  const size_t n_back = 4 * (size_t)mt_max_parts(cfg->max_query) * (size_t)cfg->max_train;
  const size_t n_merged = 3 * (size_t)cfg->max_query, n_merged_back = (size_t)cfg->max_train;
  const size_t n_blocks = ((size_t)cfg->max_query + kPcThreads - 1) / kPcThreads;
  if (hipSetDevice(cfg->device) != hipSuccess ||
      hipMalloc((void**)&c->part, sizeof(int32_t) * (n_part + n_back + n_merged + n_merged_back + n_blocks)) != hipSuccess) {
    c->part = nullptr;
    gcs_match_ctx_destroy(c);
    return GCS_ERR_HIP;
  }
  c->part_back = c->part + n_part;
  c->merged = c->part_back + n_back;
  c->merged_back = c->merged + n_merged;
  c->block_count = c->merged_back + n_merged_back;
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

// ---- the gated matcher and the pairs

int gcs_match_gate_defaults(gcs_match_gate* g) {
  if (!g) return GCS_ERR_ARG;
  memset(g, 0, sizeof(*g));
  g->radius = 16.0f;
  g->max_level_diff = 1;
  return GCS_OK;
}

int gcs_match_filter_defaults(gcs_match_filter* f) {
  if (!f) return GCS_ERR_ARG;
  f->max_distance = 64;
  f->ratio_num = 4;
  f->ratio_den = 5;
  f->cross_check = 1;
  return GCS_OK;
}

}  // extern "C"

namespace {

// D8 of query row i on the host: the candidates in ascending j
void mt_host_forward(const gcs_match_inputs* in, const gcs_match_gate* g, int i, int* idx, int* dist, int* dist2, int* n_cand) {
  *dist = *dist2 = kKdNoMatch;
  *idx = -1;
  *n_cand = 0;
  for (int j = 0; j < in->n_train; ++j)
    if (mt_host_candidate(in, g, i, j)) {
      ++*n_cand;
      kd_match_step(mt_host_distance(in, i, j), j, dist, idx, dist2);
    }
}

// the forward and backward searches of a call as the kernels see them
MtSearches mt_searches(gcs_match_ctx* c, const gcs_match_inputs* in, const gcs_match_gate* g) {
  MtSearches p;
  memset(&p, 0, sizeof(p));
  MtSearch &f = p.s[0], &b = p.s[1];
  f.q = (const uint32_t*)in->q;
  f.t = (const uint32_t*)in->t;
  f.q_bin = in->q_bin;
  f.t_bin = in->t_bin;
  f.n_q = in->n_query;
  f.n_t = in->n_train;
  if (g) {
    f.q_u = g->q_pu ? g->q_pu : g->q_u;
    f.q_v = g->q_pv ? g->q_pv : g->q_v;
    f.q_level = g->q_level;
    f.t_u = g->t_u;
    f.t_v = g->t_v;
    f.t_level = g->t_level;
    p.radius = g->radius;
    p.max_level_diff = g->max_level_diff;
  }
  mt_split(f.n_t, &f.chunk, &f.parts);
  f.part = c->part;
  b.q = f.t;
  b.t = f.q;
  b.q_bin = f.t_bin;
  b.t_bin = f.q_bin;
  b.q_u = f.t_u;
  b.q_v = f.t_v;
  b.q_level = f.t_level;
  b.t_u = f.q_u;
  b.t_v = f.q_v;
  b.t_level = f.q_level;
  b.n_q = f.n_t;
  b.n_t = f.n_q;
  mt_split(b.n_t, &b.chunk, &b.parts);
  b.part = c->part_back;
  return p;
}

// the searches of `dirs` directions in one launch, their merges in another
void mt_launch_searches(gcs_match_ctx* c, const MtSearches& p, int dirs, bool gate) {
  int rows = p.s[0].n_q, parts = p.s[0].parts;
  if (dirs == 2) {
    rows = std::max(rows, p.s[1].n_q);
    parts = std::max(parts, p.s[1].parts);
  }
  const int blocks = std::max(1, (rows + kMtThreads - 1) / kMtThreads);
  if (gate)
    hipLaunchKernelGGL(k_match_gated_partial<true>, dim3(blocks, parts, dirs), dim3(kMtThreads), 0, c->stream, p);
  else
    hipLaunchKernelGGL(k_match_gated_partial<false>, dim3(blocks, parts, dirs), dim3(kMtThreads), 0, c->stream, p);
  hipLaunchKernelGGL(k_match_gated_merge, dim3(blocks, 1, dirs), dim3(kMtThreads), 0, c->stream, p);
}

}  // namespace

extern "C" {

int gcs_match_descriptors_gated_host(const gcs_match_config* cfg, const gcs_match_inputs* in, const gcs_match_gate* gate,
                                     gcs_match_gated_outputs* out) {
  if (mt_check_config(cfg) || mt_check_gated(*cfg, in, gate, out)) return GCS_ERR_ARG;
  for (int i = 0; i < in->n_query; ++i) {
    int idx, dist, dist2, n_cand;
    mt_host_forward(in, gate, i, &idx, &dist, &dist2, &n_cand);
    out->idx[i] = idx;
    out->dist[i] = dist;
    out->dist2[i] = dist2;
    if (out->n_cand) out->n_cand[i] = n_cand;
  }
  return GCS_OK;
}

int gcs_match_pairs_host(const gcs_match_config* cfg, const gcs_match_inputs* in, const gcs_match_gate* gate,
                         const gcs_match_filter* f, gcs_match_pair_outputs* out) {
  if (mt_check_config(cfg) || mt_check_pairs(*cfg, in, gate, f, out)) return GCS_ERR_ARG;
  int count = 0;
  for (int i = 0; i < in->n_query; ++i) {
    int idx, dist, dist2, n_cand;
    mt_host_forward(in, gate, i, &idx, &dist, &dist2, &n_cand);
    bool keep = kd_pair_filters(idx, dist, dist2, f->max_distance, f->ratio_num, f->ratio_den);
    if (keep && f->cross_check) {   // the backward search of train row idx: the query rows k with C(k, idx), by (distance, lowest k)
      int b_dist = kKdNoMatch, b_idx = -1, b_dist2 = kKdNoMatch;
      for (int k = 0; k < in->n_query; ++k)
        if (mt_host_candidate(in, gate, k, idx)) kd_match_step(mt_host_distance(in, k, idx), k, &b_dist, &b_idx, &b_dist2);
      keep = b_idx == i;
    }
    if (keep) {
      out->pair_a[count] = i;
      out->pair_b[count] = idx;
      out->pair_dist[count] = dist;
      ++count;
    }
  }
  for (int i = count; i < in->n_query; ++i) {
    out->pair_a[i] = out->pair_b[i] = -1;
    out->pair_dist[i] = kKdNoMatch;
  }
  *out->count = count;
  return GCS_OK;
}

int gcs_match_descriptors_gated(gcs_match_ctx* c, const gcs_match_inputs* in, const gcs_match_gate* gate,
                                gcs_match_gated_outputs* out) {
  if (!c) return GCS_ERR_ARG;
  if (const char* m = mt_check_gated(c->cfg, in, gate, out)) return mt_fail(c, GCS_ERR_ARG, m);
  if (in->n_query == 0) return GCS_OK;
  KDCHK(mt_fail, c, hipSetDevice(c->device));
  MtSearches p = mt_searches(c, in, gate);
  p.s[0].idx = out->idx;
  p.s[0].dist = out->dist;
  p.s[0].dist2 = out->dist2;
  p.s[0].n_cand = out->n_cand;
  mt_launch_searches(c, p, 1, true);
  KDCHK(mt_fail, c, hipGetLastError());
  return GCS_OK;
}

int gcs_match_pairs(gcs_match_ctx* c, const gcs_match_inputs* in, const gcs_match_gate* gate, const gcs_match_filter* f,
                    gcs_match_pair_outputs* out) {
  if (!c) return GCS_ERR_ARG;
  if (const char* m = mt_check_pairs(c->cfg, in, gate, f, out)) return mt_fail(c, GCS_ERR_ARG, m);
  KDCHK(mt_fail, c, hipSetDevice(c->device));
  const int n_q = in->n_query;
  if (n_q == 0) {
    KDCHK(mt_fail, c, hipMemsetAsync(out->count, 0, sizeof(int32_t), c->stream));
    return GCS_OK;
  }
  MtSearches p = mt_searches(c, in, gate);
  p.s[0].idx = c->merged;
  p.s[0].dist = c->merged + n_q;
  p.s[0].dist2 = c->merged + 2 * (size_t)n_q;
  p.s[1].idx = c->merged_back;
  mt_launch_searches(c, p, f->cross_check ? 2 : 1, gate != nullptr);
  MtPairs w;
  memset(&w, 0, sizeof(w));
  w.idx = p.s[0].idx;
  w.dist = p.s[0].dist;
  w.dist2 = p.s[0].dist2;
  w.back = c->merged_back;
  w.n_q = n_q;
  w.n_blocks = (n_q + kPcThreads - 1) / kPcThreads;
  w.f = *f;
  w.f.cross_check = f->cross_check ? 1 : 0;
  w.block_count = c->block_count;
  w.o = *out;
  if (w.n_blocks > 1) hipLaunchKernelGGL(k_pairs_count, dim3(w.n_blocks), dim3(kPcThreads), 0, c->stream, w);
  hipLaunchKernelGGL(k_pairs_write, dim3(w.n_blocks), dim3(kPcThreads), 0, c->stream, w);
  KDCHK(mt_fail, c, hipGetLastError());
  return GCS_OK;
}

}  // extern "C"
