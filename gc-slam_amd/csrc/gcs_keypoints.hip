// Keypoints on the GPU: the detector front of the FAST / ORB recipe at pyramid level 0, from an 8-bit image to
// the (kp_u, kp_v, kp_response) arrays gcs_visfeat_inputs reads.  The project's own definition
// (include/gcslam_hip.h): no pyramid, and no parity with cv::ORB; orientation and descriptors are
// gcs_descriptors.hip's.  Kernels:
//   k_kp_score     one 64 x 16 tile per workgroup: the tile's bytes with a 3-pixel halo into LDS as whole dwords
//                  (bytes only where a dword would leave the row), grey from rgb there, then per pixel the
//                  bright / dark ring masks, the 9-run gate and, behind it, the FAST score; writes the grey
//                  image and the one-byte score image, every pixel of W x H
//   k_kp_response  one tile per workgroup: strict 3 x 3 suppression on the score tile and the border rule; the
//                  survivors are listed in LDS and each is handed to a wave, one lane per pixel of the 7 x 7
//                  block, integer butterfly sums; writes the dense key image (0: no keypoint), every pixel, and
//                  the histogram of the keys' top byte
//   k_kp_hist      x 3: the radix select's next byte, over the keys that share the bytes chosen so far
//   k_kp_count     resolves the last byte: the max_keypoints-th largest key `kth`; per strip of 2048 pixels the
//                  number of keys above it and equal to it
//   k_kp_scan      one workgroup over the strips' counts (not over the image): exclusive offsets, `counts`,
//                  the NaN padding
//   k_kp_emit      per strip: the kept pixels in raster order, ties on kth to the lowest raster indices
// Histograms are per workgroup in LDS and merged with integer atomics, so every run gives the same bytes.
// Each select kernel redoes the 256-bin suffix scan of the byte before it, so no launch exists only to
// pick a bin.  The math is gcs_keypoints_math.h, which gcs_detect_keypoints_host runs on the host.
//
// gcs_detect_keypoints_pyramid runs the same detector over a scale pyramid (the definition: P1-P5 in
// include/gcslam_hip.h) in one memset and nine launches whatever n_levels is: the levels' grey, score and key
// images are packed one after another (KpLevels), the bodies of the kernels above are __device__ functions of a
// tile or a strip, and the k_kpp_* kernels look their level up from blockIdx.x:
//   k_kpp_resample every level's grey image from the input (level 0: the grey conversion; level l: the exact
//                  pixel-area mean over its footprint, in integers)
//   k_kpp_score, k_kpp_response, k_kpp_hist x 3, k_kpp_count   the tile / strip functions on the block's level,
//                  with per-level histograms, select state and quota
//   k_kpp_scan     one workgroup over all levels' strips; per-level and total counts, each level's first row
//   k_kpp_emit     level-major, raster-within-level rows in level-0 coordinates, with kp_level
//
// gcs_detect_keypoints_grid replaces the pyramid's per-level select by a fair share among the cells of a grid
// over each level and hands a level's unused quota on (the definition: G1-G4 in include/gcslam_hip.h): the
// k_kpg_* kernels further down, one memset and twelve launches whatever n_levels and the number of cells are.

#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <functional>
#include <string>
#include <vector>

#include "gcs_keypoints_levels.h"
#include "gcs_keypoints_math.h"
#include "gcslam_hip.h"

#pragma clang fp contract(off)

namespace gcs {
namespace {

// (kKpTileW, kKpTileH, kKpThreads and kKpStrip: gcs_keypoints_levels.h)
constexpr int kKpRows = kKpTileH / (kKpThreads / kKpTileW);   // pixels per thread, one per 4 rows
constexpr int kKpGW = kKpTileW + 2 * kKpFrame, kKpGH = kKpTileH + 2 * kKpFrame, kKpGStride = 72;
constexpr int kKpRawDw = 56;       // dwords per staged row: 3 * 70 bytes and up to 3 in front of them, 54 dwords
constexpr int kKpSW = kKpTileW + 2, kKpSH = kKpTileH + 2, kKpSStride = 68;
constexpr int kKpPerThread = kKpStrip / kKpThreads;
constexpr int kKpScanThreads = 1024;
constexpr int kKpBins = 256;

struct KpSel {          // the radix select's state after a byte
  uint32_t prefix;      // the bytes chosen so far, in place
  int32_t rem;          // the rank still looked for among the keys that share them (1-based, from the top)
  int32_t all;          // no more survivors than max_keypoints: every one is kept
  int32_t total;        // survivors
};

struct KpWork {
  uint8_t *grey, *score;
  uint32_t* key;
  uint32_t* hist;       // 4 x 256 bins, then n_corners
  KpSel* st;            // [1..4]: after each byte
  int2 *strip_cnt, *strip_off;
};

// ---- k_kp_score

// The tile at (x0, y0) of a W x H image, by one workgroup; a kernel calls it once.  GREY_OUT false: img is the
// grey image itself (CH 1) and is not written again.  The LDS arrays of this and the other per-tile and
// per-strip functions are declared inside them, not handed in by pointer: through a generic pointer the compiler
// folded k_kp_response's list store and its key store into one flat store, and list entries written that way
// were not all seen behind the barrier on gfx950 (counts changed from run to run).
template <int CH, bool GREY_OUT>
__device__ __forceinline__ void kp_score_tile(const uint8_t* __restrict__ img, int64_t pitch, int W, int H, int threshold,
                                              uint8_t* __restrict__ grey_out, uint8_t* __restrict__ score_out,
                                              uint32_t* __restrict__ n_corners, int x0, int y0) {
  __shared__ uint32_t raw[kKpGH * kKpRawDw];
  __shared__ uint8_t grey[kKpGH * kKpGStride];
  const int t = threadIdx.x;
  const int xa = max(x0 - kKpFrame, 0), xb = min(x0 + kKpTileW + kKpFrame, W);   // the tile's columns inside the image
  for (int idx = t; idx < kKpGH * kKpRawDw; idx += kKpThreads) {
    const int r = idx / kKpRawDw, i = idx % kKpRawDw;
    const int y = y0 - kKpFrame + r;
    uint32_t v = 0;
    if (y >= 0 && y < H) {
      const uintptr_t row = (uintptr_t)img + (uintptr_t)((int64_t)y * pitch);
      const uintptr_t a = row + (uintptr_t)(CH * xa), e = row + (uintptr_t)(CH * xb);   // the bytes wanted: [a, e)
      const uintptr_t q = (a & ~(uintptr_t)3) + 4u * (uintptr_t)i;
      if (q >= a && q + 4 <= e) {
        v = *(const uint32_t*)q;
      } else if (q < e && q + 4 > a) {   // a dword that leaves the row's pixels: its bytes inside, one by one
        for (int k = 0; k < 4; ++k)
          if (q + k >= a && q + k < e) v |= (uint32_t)(*(const uint8_t*)(q + k)) << (8 * k);
      }
    }
    raw[idx] = v;
  }
  __syncthreads();
  for (int idx = t; idx < kKpGH * kKpGW; idx += kKpThreads) {
    const int r = idx / kKpGW, c = idx % kKpGW;
    const int x = x0 - kKpFrame + c, y = y0 - kKpFrame + r;
    int g = 0;
    if (x >= 0 && x < W && y >= 0 && y < H) {
      const uintptr_t a = (uintptr_t)img + (uintptr_t)((int64_t)y * pitch) + (uintptr_t)(CH * xa);
      const uint8_t* b = (const uint8_t*)&raw[r * kKpRawDw] + (int)(a & 3) + CH * (x - xa);
      g = CH == 3 ? kp_grey(b[0], b[1], b[2]) : b[0];
    }
    grey[r * kKpGStride + c] = (uint8_t)g;
  }
  __syncthreads();
  const int lx = t & (kKpTileW - 1), x = x0 + lx;
  int corners = 0;
#pragma unroll
  for (int k = 0; k < kKpRows; ++k) {
    const int ly = (t >> 6) + k * (kKpThreads / kKpTileW), y = y0 + ly;
    if (x < W && y < H) {
      const uint8_t* c = &grey[(ly + kKpFrame) * kKpGStride + lx + kKpFrame];
      int s = 0;
      if (x >= kKpFrame && x < W - kKpFrame && y >= kKpFrame && y < H - kKpFrame) s = kp_fast_score(c, kKpGStride, threshold);
      if (GREY_OUT) grey_out[y * W + x] = c[0];
      score_out[y * W + x] = (uint8_t)s;
      corners += s > 0;
    }
  }
  for (int off = 32; off > 0; off >>= 1) corners += __shfl_xor(corners, off, 64);
  if ((t & 63) == 0 && corners) atomicAdd(n_corners, (uint32_t)corners);
}

template <int CH>
__global__ __launch_bounds__(kKpThreads) void k_kp_score(const uint8_t* __restrict__ img, int64_t pitch, int W, int H,
                                                         int threshold, uint8_t* __restrict__ grey_out,
                                                         uint8_t* __restrict__ score_out, uint32_t* __restrict__ n_corners) {
  kp_score_tile<CH, true>(img, pitch, W, H, threshold, grey_out, score_out, n_corners, blockIdx.x * kKpTileW,
                          blockIdx.y * kKpTileH);
}

// ---- k_kp_response

// the tile at (x0, y0) of a W x H image; ghist: the 256 bins of the keys' top byte
__device__ __forceinline__ void kp_response_tile(const uint8_t* __restrict__ score, const uint8_t* __restrict__ grey, int W,
                                                 int H, int edge, double harris_k, uint32_t* __restrict__ key,
                                                 uint32_t* __restrict__ ghist, int x0, int y0) {
  __shared__ uint8_t sc[kKpSH * kKpSStride];
  __shared__ int list[kKpTileW * kKpTileH];
  __shared__ int n_list;
  __shared__ uint32_t hist[kKpBins];
  const int t = threadIdx.x;
  for (int idx = t; idx < kKpSH * kKpSW; idx += kKpThreads) {
    const int r = idx / kKpSW, c = idx % kKpSW;
    const int x = x0 - 1 + c, y = y0 - 1 + r;
    sc[r * kKpSStride + c] = (x >= 0 && x < W && y >= 0 && y < H) ? score[y * W + x] : (uint8_t)0;
  }
  hist[t] = 0;
  if (t == 0) n_list = 0;
  __syncthreads();
  const int lx = t & (kKpTileW - 1), x = x0 + lx;
#pragma unroll
  for (int k = 0; k < kKpRows; ++k) {
    const int ly = (t >> 6) + k * (kKpThreads / kKpTileW), y = y0 + ly;
    if (x < W && y < H) {
      const uint8_t* c = &sc[(ly + 1) * kKpSStride + lx + 1];
      const int s = c[0];
      const bool peak = s > 0 && s > c[-kKpSStride - 1] && s > c[-kKpSStride] && s > c[-kKpSStride + 1] && s > c[-1] &&
                        s > c[1] && s > c[kKpSStride - 1] && s > c[kKpSStride] && s > c[kKpSStride + 1];
      if (peak && x >= edge && x < W - edge && y >= edge && y < H - edge)
        list[atomicAdd(&n_list, 1)] = (ly << 8) | lx;   // (at most one per pixel of the tile: it cannot overflow)
      else
        key[y * W + x] = 0;
    }
  }
  __syncthreads();
  const int n = n_list, lane = t & 63;
  for (int i = t >> 6; i < n; i += kKpThreads / 64) {   // uniform over the wave
    const int px = x0 + (list[i] & 255), py = y0 + (list[i] >> 8);
    int a = 0, b = 0, c = 0;
    if (lane < kKpBlock * kKpBlock) {   // edge >= 4: the block and its Sobel taps are inside the image
      int ix, iy;
      kp_sobel(grey + (py + lane / kKpBlock - kKpBlock / 2) * W + (px + lane % kKpBlock - kKpBlock / 2), W, &ix, &iy);
      a = ix * ix; b = iy * iy; c = ix * iy;   // |I| <= 1020: 49 squares stay below 2^26
    }
    for (int off = 32; off > 0; off >>= 1) {
      a += __shfl_xor(a, off, 64);
      b += __shfl_xor(b, off, 64);
      c += __shfl_xor(c, off, 64);
    }
    if (lane == 0) {
      const uint32_t kk = kp_key_of_bits(__float_as_uint(kp_response(a, b, c, harris_k)));
      key[py * W + px] = kk;
      atomicAdd(&hist[kk >> 24], 1u);
    }
  }
  __syncthreads();
  if (hist[t]) atomicAdd(&ghist[t], hist[t]);
}

__global__ __launch_bounds__(kKpThreads) void k_kp_response(const uint8_t* __restrict__ score, const uint8_t* __restrict__ grey,
                                                            int W, int H, int edge, double harris_k,
                                                            uint32_t* __restrict__ key, uint32_t* __restrict__ ghist) {
  kp_response_tile(score, grey, W, H, edge, harris_k, key, ghist, blockIdx.x * kKpTileW, blockIdx.y * kKpTileH);
}

// ---- the select

// Byte q of the select from its histogram (counts of that byte over the keys sharing prev.prefix's higher
// bytes): the bin that holds rank prev.rem from the top.  Every thread of the 256 gets the result.
__device__ KpSel kp_resolve(const uint32_t* __restrict__ hist_q, KpSel prev, int q, uint32_t* s, KpSel* box) {
  if (prev.all) return prev;
  const int t = threadIdx.x;
  s[t] = hist_q[kKpBins - 1 - t];   // from the top bin down
  __syncthreads();
  for (int off = 1; off < kKpBins; off <<= 1) {
    const uint32_t add = t >= off ? s[t - off] : 0u;
    __syncthreads();
    s[t] += add;
    __syncthreads();
  }
  const uint32_t incl = s[t], below = t ? s[t - 1] : 0u, total = s[kKpBins - 1], rem = (uint32_t)prev.rem;
  const bool all = q == 0 && total <= rem;
  if (t == 0) {
    box->all = all;
    box->total = q == 0 ? (int32_t)total : prev.total;
    if (all) { box->prefix = 0; box->rem = 0; }
  }
  if (!all && incl >= rem && below < rem) {   // one thread
    box->prefix = prev.prefix | ((uint32_t)(kKpBins - 1 - t) << (24 - 8 * q));
    box->rem = (int32_t)(rem - below);
  }
  __syncthreads();
  const KpSel cur = *box;
  __syncthreads();
  return cur;
}

// a thread's keys of strip `strip`: [strip * 2048 + 8 t, + 8), zeros beyond n (the allocation is whole strips)
__device__ inline int kp_load_keys(const uint32_t* __restrict__ key, int strip, int n, uint32_t* k) {
  const int i0 = strip * kKpStrip + threadIdx.x * kKpPerThread;
  const uint4 lo = *(const uint4*)(key + i0), hi = *(const uint4*)(key + i0 + 4);
  const uint32_t v[kKpPerThread] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
  for (int j = 0; j < kKpPerThread; ++j) k[j] = i0 + j < n ? v[j] : 0u;
  return i0;
}

// One strip of a key image of n keys in pass `pass` of the select of the K largest; ghist: 4 x 256 bins, st: [1..4].
__device__ __forceinline__ void kp_hist_strip(const uint32_t* __restrict__ key, int strip, int n, int K, int pass,
                                              uint32_t* __restrict__ ghist, KpSel* __restrict__ st) {
  __shared__ uint32_t s[kKpBins];
  __shared__ KpSel box;
  const int t = threadIdx.x;
  const KpSel first = {0u, K, 0, 0};
  const KpSel cur = kp_resolve(ghist + (pass - 1) * kKpBins, pass == 1 ? first : st[pass - 1], pass - 1, s, &box);
  if (strip == 0 && t == 0) st[pass] = cur;
  if (cur.all) return;
  s[t] = 0;
  __syncthreads();
  uint32_t k[kKpPerThread];
  kp_load_keys(key, strip, n, k);
  const int shift = 32 - 8 * pass;
#pragma unroll
  for (int j = 0; j < kKpPerThread; ++j)   // (a key of 0 shares no chosen byte: the top byte of a real key is never 0)
    if (k[j] && (k[j] >> shift) == (cur.prefix >> shift)) atomicAdd(&s[(k[j] >> (shift - 8)) & 255u], 1u);
  __syncthreads();
  if (s[t]) atomicAdd(&ghist[pass * kKpBins + t], s[t]);
}

__global__ __launch_bounds__(kKpThreads) void k_kp_hist(const uint32_t* __restrict__ key, int n, int K, int pass,
                                                        uint32_t* __restrict__ ghist, KpSel* __restrict__ st) {
  kp_hist_strip(key, blockIdx.x, n, K, pass, ghist, st);
}

__device__ inline int kp_wave_incl(int x) {
  const int lane = threadIdx.x & 63;
  for (int off = 1; off < 64; off <<= 1) {
    const int y = __shfl_up(x, off, 64);
    if (lane >= off) x += y;
  }
  return x;
}

// The cut of a finished select: keys above kth are kept, and of the keys equal to it the first `need` in raster
// order.  A quota of 0 (a pyramid level's; the select then ran for rank 1) keeps nothing: no finite
// response has the key 0xffffffff.
__device__ inline void kp_cut(const KpSel cur, int quota, uint32_t* kth, int* need) {
  *kth = quota == 0 ? 0xffffffffu : cur.all ? 0u : cur.prefix;
  *need = (quota == 0 || cur.all) ? 0 : cur.rem;
}
__device__ inline int kp_kept(const KpSel cur, int quota) { return quota == 0 ? 0 : cur.all ? cur.total : quota; }

// resolves the last byte and counts one strip; cnt: the strip's (above kth, equal to kth)
__device__ __forceinline__ void kp_count_strip(const uint32_t* __restrict__ key, int strip, int n, int quota,
                                               const uint32_t* __restrict__ ghist, KpSel* __restrict__ st,
                                               int2* __restrict__ cnt) {
  __shared__ uint32_t s[kKpBins];
  __shared__ KpSel box;
  __shared__ int2 part[kKpThreads / 64];
  const int t = threadIdx.x;
  const KpSel cur = kp_resolve(ghist + 3 * kKpBins, st[3], 3, s, &box);
  if (strip == 0 && t == 0) st[4] = cur;
  uint32_t kth;
  int need;
  kp_cut(cur, quota, &kth, &need);
  uint32_t k[kKpPerThread];
  kp_load_keys(key, strip, n, k);
  int gt = 0, eq = 0;
#pragma unroll
  for (int j = 0; j < kKpPerThread; ++j) {
    gt += k[j] > kth;
    eq += k[j] == kth;
  }
  for (int off = 32; off > 0; off >>= 1) {
    gt += __shfl_xor(gt, off, 64);
    eq += __shfl_xor(eq, off, 64);
  }
  if ((t & 63) == 0) part[t >> 6] = make_int2(gt, eq);
  __syncthreads();
  if (t == 0) {
    int2 c = part[0];
    for (int w = 1; w < kKpThreads / 64; ++w) { c.x += part[w].x; c.y += part[w].y; }
    *cnt = c;
  }
}

__global__ __launch_bounds__(kKpThreads) void k_kp_count(const uint32_t* __restrict__ key, int n, int K,
                                                         const uint32_t* __restrict__ ghist, KpSel* __restrict__ st,
                                                         int2* __restrict__ strip_cnt) {
  kp_count_strip(key, blockIdx.x, n, K, ghist, st, strip_cnt + blockIdx.x);
}

// exclusive offsets of the strips' counts, by one workgroup of kKpScanThreads
__device__ __forceinline__ void kp_scan_strips(const int2* __restrict__ strip_cnt, int n_strips, int2* __restrict__ strip_off) {
  __shared__ int sg[kKpScanThreads], se[kKpScanThreads];
  const int t = threadIdx.x;
  const int per = (n_strips + kKpScanThreads - 1) / kKpScanThreads;
  const int lo = min(n_strips, t * per), hi = min(n_strips, lo + per);
  int g = 0, e = 0;
  for (int i = lo; i < hi; ++i) { g += strip_cnt[i].x; e += strip_cnt[i].y; }
  sg[t] = g; se[t] = e;
  __syncthreads();
  for (int off = 1; off < kKpScanThreads; off <<= 1) {
    const int ag = t >= off ? sg[t - off] : 0, ae = t >= off ? se[t - off] : 0;
    __syncthreads();
    sg[t] += ag; se[t] += ae;
    __syncthreads();
  }
  g = sg[t] - g; e = se[t] - e;
  for (int i = lo; i < hi; ++i) {
    strip_off[i] = make_int2(g, e);
    g += strip_cnt[i].x; e += strip_cnt[i].y;
  }
}

__global__ __launch_bounds__(kKpScanThreads) void k_kp_scan(const int2* __restrict__ strip_cnt, int n_strips,
                                                            const KpSel* __restrict__ st, const uint32_t* __restrict__ n_corners,
                                                            int2* __restrict__ strip_off, int K, gcs_keypoint_outputs o) {
  const int t = threadIdx.x;
  kp_scan_strips(strip_cnt, n_strips, strip_off);
  const KpSel cur = st[4];
  const int n_kp = cur.all ? cur.total : K;
  if (t == 0) {
    o.counts[0] = n_kp;
    o.counts[1] = cur.total;
    o.counts[2] = (int32_t)*n_corners;
    o.counts[3] = 0;
  }
  for (int i = n_kp + t; i < K; i += kKpScanThreads) o.kp_u[i] = o.kp_v[i] = o.kp_response[i] = NAN;
}

// Where a kept pixel goes.  The single-level detector: its own coordinates.  A pyramid level of size Wl x Hl under
// a W0 x H0 image: the level-0 coordinates of the pixel's centre, and the level.
struct KpPlace {
  int Wl, Hl, W0, H0, level;
  int32_t* kp_level;   // null: the single-level detector
};

// One strip of a key image n keys long and Wl wide: the kept pixels in raster order at rows first + (the strip's
// offsets `base` among the keys above and equal to kth); rows from K on are not written.
// SPLIT (the grid detector): `key` decides and the response is read from resp_key, the image of the responses' keys.
template <bool SPLIT = false>
__device__ __forceinline__ void kp_emit_strip(const uint32_t* __restrict__ key, int strip, int n, uint32_t kth, int need,
                                              int2 base, int first, int K, float* __restrict__ kp_u, float* __restrict__ kp_v,
                                              float* __restrict__ kp_response, const KpPlace pl,
                                              const uint32_t* __restrict__ resp_key = nullptr) {
  __shared__ int2 part[kKpThreads / 64];
  const int t = threadIdx.x;
  uint32_t k[kKpPerThread], r[kKpPerThread];
  const int i0 = kp_load_keys(key, strip, n, k);
  if (SPLIT) kp_load_keys(resp_key, strip, n, r);
  int gt = 0, eq = 0;
#pragma unroll
  for (int j = 0; j < kKpPerThread; ++j) {
    gt += k[j] > kth;
    eq += k[j] == kth;
  }
  const int ig = kp_wave_incl(gt), ie = kp_wave_incl(eq);
  if ((t & 63) == 63) part[t >> 6] = make_int2(ig, ie);
  __syncthreads();
  for (int w = 0; w < (t >> 6); ++w) { base.x += part[w].x; base.y += part[w].y; }
  int g = base.x + ig - gt, e = base.y + ie - eq;   // keys above / equal to kth before this thread's, in raster order
#pragma unroll
  for (int j = 0; j < kKpPerThread; ++j) {
    const bool above = k[j] > kth, tie = k[j] == kth;
    if (above || (tie && e < need)) {
      const int pos = first + g + min(e, need), i = i0 + j;
      if (pos < K) {
        if (pl.kp_level) {
          kp_u[pos] = kp_level0_coord(i % pl.Wl, pl.W0, pl.Wl);
          kp_v[pos] = kp_level0_coord(i / pl.Wl, pl.H0, pl.Hl);
          pl.kp_level[pos] = pl.level;
        } else {
          kp_u[pos] = (float)(i % pl.Wl);
          kp_v[pos] = (float)(i / pl.Wl);
        }
        kp_response[pos] = __uint_as_float(kp_bits_of_key(SPLIT ? r[j] : k[j]));
      }
    }
    g += above;
    e += tie;
  }
}

__global__ __launch_bounds__(kKpThreads) void k_kp_emit(const uint32_t* __restrict__ key, int n, int W,
                                                        const KpSel* __restrict__ st, const int2* __restrict__ strip_off,
                                                        int K, gcs_keypoint_outputs o) {
  uint32_t kth;
  int need;   // of the keys equal to kth, the first `need` in raster order are kept
  kp_cut(st[4], K, &kth, &need);
  const KpPlace pl = {W, 0, 0, 0, 0, nullptr};
  kp_emit_strip(key, blockIdx.x, n, kth, need, strip_off[blockIdx.x], 0, K, o.kp_u, o.kp_v, o.kp_response, pl);
}

// ---- the pyramid (gcs_detect_keypoints_pyramid)
//
// The level table (KpLevels, kp_levels), its lookups (kp_level_at, kp_pick), kp_resample_pixel and
// k_kpp_resample are in gcs_keypoints_levels.h, which the describer shares.

// k_kp_score over the tiles of all levels, from the packed grey image
__global__ __launch_bounds__(kKpThreads) void k_kpp_score(const uint8_t* __restrict__ grey_in, const KpLevels lv, int threshold,
                                                          uint8_t* __restrict__ score_out, uint32_t* __restrict__ n_corners) {
  const int l = kp_level_at(lv.tile0, lv.n, blockIdx.x);
  const int Wl = kp_pick(lv.W, l), Hl = kp_pick(lv.H, l), tx = kp_pick(lv.tiles_x, l);
  const int tile = blockIdx.x - kp_pick(lv.tile0, l);
  const size_t px = (size_t)kp_pick(lv.block0, l) * kKpThreads;
  kp_score_tile<1, false>(grey_in + px, Wl, Wl, Hl, threshold, nullptr, score_out + px, n_corners + l,
                          (tile % tx) * kKpTileW, (tile / tx) * kKpTileH);
}

// k_kp_response over the tiles of all levels; ghist: per level 4 x 256 bins
__global__ __launch_bounds__(kKpThreads) void k_kpp_response(const uint8_t* __restrict__ score, const uint8_t* __restrict__ grey,
                                                             const KpLevels lv, int edge, double harris_k,
                                                             uint32_t* __restrict__ key, uint32_t* __restrict__ ghist) {
  const int l = kp_level_at(lv.tile0, lv.n, blockIdx.x);
  const int Wl = kp_pick(lv.W, l), Hl = kp_pick(lv.H, l), tx = kp_pick(lv.tiles_x, l);
  const int tile = blockIdx.x - kp_pick(lv.tile0, l);
  const size_t px = (size_t)kp_pick(lv.block0, l) * kKpThreads;
  kp_response_tile(score + px, grey + px, Wl, Hl, edge, harris_k, key + (size_t)kp_pick(lv.strip0, l) * kKpStrip,
                   ghist + l * 4 * kKpBins, (tile % tx) * kKpTileW, (tile / tx) * kKpTileH);
}

// The select, segmented: strip blockIdx.x belongs to one level, whose histograms, state (st + 5 l) and quota it
// uses.  A quota of 0 runs the select for rank 1 and is cut to nothing afterwards (kp_cut).
__global__ __launch_bounds__(kKpThreads) void k_kpp_hist(const uint32_t* __restrict__ key, const KpLevels lv, int pass,
                                                         uint32_t* __restrict__ ghist, KpSel* __restrict__ st) {
  const int l = kp_level_at(lv.strip0, lv.n, blockIdx.x), first = kp_pick(lv.strip0, l);
  kp_hist_strip(key + (size_t)first * kKpStrip, blockIdx.x - first, kp_pick(lv.W, l) * kp_pick(lv.H, l),
                max(kp_pick(lv.quota, l), 1), pass, ghist + l * 4 * kKpBins, st + 5 * l);
}

__global__ __launch_bounds__(kKpThreads) void k_kpp_count(const uint32_t* __restrict__ key, const KpLevels lv,
                                                          const uint32_t* __restrict__ ghist, KpSel* __restrict__ st,
                                                          int2* __restrict__ strip_cnt) {
  const int l = kp_level_at(lv.strip0, lv.n, blockIdx.x), first = kp_pick(lv.strip0, l);
  kp_count_strip(key + (size_t)first * kKpStrip, blockIdx.x - first, kp_pick(lv.W, l) * kp_pick(lv.H, l),
                 kp_pick(lv.quota, l), ghist + l * 4 * kKpBins, st + 5 * l, strip_cnt + blockIdx.x);
}

// One workgroup over all levels' strips: the offsets run through the levels, so a strip's offset within its
// level is its own less its level's first strip's.  Then each level's counts, its first output row
// (level_row), the totals and the padding.
__global__ __launch_bounds__(kKpScanThreads) void k_kpp_scan(const int2* __restrict__ strip_cnt, const KpLevels lv,
                                                             const KpSel* __restrict__ st, const uint32_t* __restrict__ n_corners,
                                                             int2* __restrict__ strip_off, int32_t* __restrict__ level_row, int K,
                                                             gcs_keypoint_pyramid_outputs o) {
  __shared__ int n_all;
  const int t = threadIdx.x;
  kp_scan_strips(strip_cnt, lv.strip0[kKpMaxLevels], strip_off);
  if (t == 0) {
    int row = 0, survivors = 0, corners = 0;
#pragma unroll
    for (int l = 0; l < kKpMaxLevels; ++l) {
      int32_t c[4] = {0, 0, 0, l < lv.n ? lv.quota[l] : 0};
      if (l < lv.n && lv.strip0[l + 1] > lv.strip0[l]) {   // a level without pixels has no state
        const KpSel cur = st[5 * l + 4];
        c[0] = kp_kept(cur, lv.quota[l]);
        c[1] = cur.total;
        c[2] = (int32_t)n_corners[l];
      }
      level_row[l] = row;
      for (int j = 0; j < 4; ++j) o.level_counts[4 * l + j] = c[j];
      row += c[0]; survivors += c[1]; corners += c[2];
    }
    o.counts[0] = row;
    o.counts[1] = survivors;
    o.counts[2] = corners;
    o.counts[3] = lv.n;
    n_all = row;
  }
  __syncthreads();
  for (int i = n_all + t; i < K; i += kKpScanThreads) {
    o.kp_u[i] = o.kp_v[i] = o.kp_response[i] = NAN;
    o.kp_level[i] = -1;
  }
}

__global__ __launch_bounds__(kKpThreads) void k_kpp_emit(const uint32_t* __restrict__ key, const KpLevels lv,
                                                         const KpSel* __restrict__ st, const int2* __restrict__ strip_off,
                                                         const int32_t* __restrict__ level_row, int K,
                                                         gcs_keypoint_pyramid_outputs o) {
  const int l = kp_level_at(lv.strip0, lv.n, blockIdx.x), first = kp_pick(lv.strip0, l);
  const int Wl = kp_pick(lv.W, l), Hl = kp_pick(lv.H, l);
  uint32_t kth;
  int need;
  kp_cut(st[5 * l + 4], kp_pick(lv.quota, l), &kth, &need);
  const int2 mine = strip_off[blockIdx.x], head = strip_off[first];
  const KpPlace pl = {Wl, Hl, lv.W[0], lv.H[0], l, o.kp_level};
  kp_emit_strip(key + (size_t)first * kKpStrip, blockIdx.x - first, Wl * Hl, kth, need,
                make_int2(mine.x - head.x, mine.y - head.y), level_row[l], K, o.kp_u, o.kp_v, o.kp_response, pl);
}

// ---- the grid of cells (gcs_detect_keypoints_grid; the definition: G1-G4 in include/gcslam_hip.h)
//
// The pyramid's resample, score and response kernels as they are, then, whatever n_levels and the number of cells:
//   k_kpg_rank     one workgroup per cell of any level: the cell's non-zero keys listed in LDS (at most 1024), each
//                  ranked against the list by (key descending, raster ascending); writes the rank where the key
//                  is not 0 (into the second key image, which k_kpg_mark then rewrites in place), counts the
//                  level's cells by their number of survivors (cells_with) and its survivors
//   k_kpg_plan     one workgroup per level, 8 always: the 8 budgets from the survivor counts and the level's cap
//                  from its cells_with table (kg_plan), into device memory
//   k_kpg_mark     per strip: the second key -- 0xffffffff where rank <= t, the key itself where rank = t + 1,
//                  0 elsewhere -- with its top-byte histogram
//   k_kpg_hist x 3, k_kpg_count   the select of the b_l largest second keys, the budget read from device memory
//   k_kpg_scan     as k_kpp_scan, with the six-column level_counts
//   k_kpg_emit     decides on the second key and takes the response from the first
// The remainder rule of G3 is the select's own tie handling: the keys of rank t + 1 compete below the 0xffffffff
// block, ties on the last one to the lowest raster indices.

struct KgGrid {
  int32_t cell, edge, redistribute, n_cells;
  int32_t n_cx[kKpMaxLevels], cell0[kKpMaxLevels + 1];
};

struct KgPlan { int32_t b, t; };   // a level's budget and cap

// The cell (cx, cy) of a W x H level, by one workgroup.  Only pixels of the kept area are read.
__device__ __forceinline__ void kg_rank_cell(const uint32_t* __restrict__ key, int W, int H, int edge, int cell, int cx, int cy,
                                             uint32_t* __restrict__ rank, uint32_t* __restrict__ cells_with,
                                             uint32_t* __restrict__ surv) {
  __shared__ uint32_t lk[kKgMaxPerCell];
  __shared__ int la[kKgMaxPerCell];
  __shared__ int n_list;
  const int t = threadIdx.x;
  if (t == 0) n_list = 0;
  __syncthreads();
  const int x0 = edge + cx * cell, y0 = edge + cy * cell;
  const int w = min(cell, W - edge - x0), h = min(cell, H - edge - y0);   // the last column and row: partial cells
  for (int idx = t; idx < w * h; idx += kKpThreads) {
    const int at = (y0 + idx / w) * W + x0 + idx % w;
    const uint32_t k = key[at];
    if (k) {
      const int pos = atomicAdd(&n_list, 1);
      if (pos < kKgMaxPerCell) {   // (no two survivors are neighbours: a cell holds at most 32 x 32 of them)
        lk[pos] = k;
        la[pos] = at;
      }
    }
  }
  __syncthreads();
  const int n = min(n_list, kKgMaxPerCell);
  for (int i = t; i < n; i += kKpThreads) {
    const uint32_t k = lk[i];
    const int at = la[i];
    int r = 1;
    for (int j = 0; j < n; ++j) r += (lk[j] > k) | ((lk[j] == k) & (la[j] < at));
    rank[at] = (uint32_t)r;
  }
  if (t == 0 && n) {
    atomicAdd(&cells_with[n - 1], 1u);
    atomicAdd(surv, (uint32_t)n);
  }
}

__global__ __launch_bounds__(kKpThreads) void k_kpg_rank(const uint32_t* __restrict__ key, const KpLevels lv, const KgGrid gr,
                                                         uint32_t* __restrict__ rank, uint32_t* __restrict__ cells_with,
                                                         uint32_t* __restrict__ surv) {
  if ((int)blockIdx.x >= gr.n_cells) return;   // (an image without cells still has this launch)
  const int l = kp_level_at(gr.cell0, lv.n, blockIdx.x);
  const int c = blockIdx.x - kp_pick(gr.cell0, l), ncx = kp_pick(gr.n_cx, l);
  const size_t off = (size_t)kp_pick(lv.strip0, l) * kKpStrip;
  kg_rank_cell(key + off, kp_pick(lv.W, l), kp_pick(lv.H, l), gr.edge, gr.cell, c % ncx, c / ncx, rank + off,
               cells_with + l * kKgMaxPerCell, surv + l);
}

// inclusive sums of v over the 256 threads through s; *total: the last one.  s is free again on return.
__device__ inline uint32_t kg_block_incl(uint32_t v, uint32_t* s, uint32_t* total) {
  const int t = threadIdx.x;
  s[t] = v;
  __syncthreads();
  for (int off = 1; off < kKpThreads; off <<= 1) {
    const uint32_t add = t >= off ? s[t - off] : 0u;
    __syncthreads();
    s[t] += add;
    __syncthreads();
  }
  const uint32_t incl = s[t];
  *total = s[kKpThreads - 1];
  __syncthreads();
  return incl;
}

// Level l's budget (G2, from every level's survivors) and cap (G3, from the level's cells_with table), the same
// in every thread of every workgroup that asks.  Thread t holds n = 4 t + 1 .. 4 t + 4: C(n), the cells with at
// least n survivors, then G(n) = sum_{q <= n} C(q) = sum_c min(n_c, n); t_l counts the n with C(n) > 0 and
// G(n) <= b_l, which form a prefix of 1, 2, ...
__device__ __forceinline__ KgPlan kg_plan(const KpLevels& lv, int redistribute, int l, const uint32_t* __restrict__ surv,
                                          const uint32_t* __restrict__ cells_with) {
  __shared__ uint32_t s[kKpThreads];
  __shared__ int cap;
  const int t = threadIdx.x;
  int32_t sv[kKpMaxLevels], b[kKpMaxLevels];
#pragma unroll
  for (int m = 0; m < kKpMaxLevels; ++m) sv[m] = (int32_t)surv[m];
  kg_budgets(lv.quota, sv, redistribute, b);
  const uint32_t bl = (uint32_t)kp_pick(b, l);
  if (t == 0) cap = 0;
  const uint4 q = *(const uint4*)(cells_with + 4 * t);
  const uint32_t c[4] = {q.x, q.y, q.z, q.w};
  uint32_t cells;
  const uint32_t before = kg_block_incl(c[0] + c[1] + c[2] + c[3], s, &cells) - (c[0] + c[1] + c[2] + c[3]);
  uint32_t C[4];
  C[0] = cells - before;
#pragma unroll
  for (int j = 1; j < 4; ++j) C[j] = C[j - 1] - c[j - 1];
  uint32_t all;
  uint32_t G = kg_block_incl(C[0] + C[1] + C[2] + C[3], s, &all) - (C[0] + C[1] + C[2] + C[3]);
  int mine = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    G += C[j];
    mine += C[j] > 0 && G <= bl;
  }
  if (mine) atomicAdd(&cap, mine);
  __syncthreads();
  const KgPlan p = {(int32_t)bl, cap};
  __syncthreads();
  return p;
}

// One strip of level images n keys long: the second key from the first and the rank (held in key2, rewritten in
// place); ghist2: the 256 bins of the second keys' top byte.
__device__ __forceinline__ void kg_mark_strip(const uint32_t* __restrict__ key, uint32_t* key2, int strip, int n, int cap,
                                              uint32_t* __restrict__ ghist2) {
  __shared__ uint32_t hist[kKpBins];
  const int t = threadIdx.x;
  hist[t] = 0;
  __syncthreads();
  uint32_t k[kKpPerThread];
  const int i0 = kp_load_keys(key, strip, n, k);
  const uint4 lo = *(const uint4*)(key2 + i0), hi = *(const uint4*)(key2 + i0 + 4);
  const uint32_t r[kKpPerThread] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  uint32_t v[kKpPerThread];
#pragma unroll
  for (int j = 0; j < kKpPerThread; ++j) {   // (where the key is 0 the rank was not written: it is not looked at)
    v[j] = k[j] == 0 ? 0u : r[j] <= (uint32_t)cap ? 0xffffffffu : r[j] == (uint32_t)cap + 1u ? k[j] : 0u;
    if (v[j]) atomicAdd(&hist[v[j] >> 24], 1u);
  }
  *(uint4*)(key2 + i0) = make_uint4(v[0], v[1], v[2], v[3]);
  *(uint4*)(key2 + i0 + 4) = make_uint4(v[4], v[5], v[6], v[7]);
  __syncthreads();
  if (hist[t]) atomicAdd(&ghist2[t], hist[t]);
}

// One workgroup per level, always 8 of them.  (Rebuilding the plan in every workgroup of k_kpg_mark, the way the
// select kernels redo their suffix scan, saved this launch and cost 0.010 ms more per call on the MI355X.)
__global__ __launch_bounds__(kKpThreads) void k_kpg_plan(const KpLevels lv, int redistribute, const uint32_t* __restrict__ surv,
                                                         const uint32_t* __restrict__ cells_with, KgPlan* __restrict__ plan) {
  const int l = blockIdx.x;
  const KgPlan p = kg_plan(lv, redistribute, l, surv, cells_with + l * kKgMaxPerCell);
  if (threadIdx.x == 0) plan[l] = p;
}

__global__ __launch_bounds__(kKpThreads) void k_kpg_mark(const uint32_t* __restrict__ key, uint32_t* key2, const KpLevels lv,
                                                         const KgPlan* __restrict__ plan, uint32_t* __restrict__ ghist2) {
  const int l = kp_level_at(lv.strip0, lv.n, blockIdx.x), first = kp_pick(lv.strip0, l);
  const size_t off = (size_t)first * kKpStrip;
  kg_mark_strip(key + off, key2 + off, blockIdx.x - first, kp_pick(lv.W, l) * kp_pick(lv.H, l), plan[l].t,
                ghist2 + l * 4 * kKpBins);
}

__global__ __launch_bounds__(kKpThreads) void k_kpg_hist(const uint32_t* __restrict__ key2, const KpLevels lv, int pass,
                                                         const KgPlan* __restrict__ plan, uint32_t* __restrict__ ghist2,
                                                         KpSel* __restrict__ st) {
  const int l = kp_level_at(lv.strip0, lv.n, blockIdx.x), first = kp_pick(lv.strip0, l);
  kp_hist_strip(key2 + (size_t)first * kKpStrip, blockIdx.x - first, kp_pick(lv.W, l) * kp_pick(lv.H, l),
                max(plan[l].b, 1), pass, ghist2 + l * 4 * kKpBins, st + 5 * l);
}

__global__ __launch_bounds__(kKpThreads) void k_kpg_count(const uint32_t* __restrict__ key2, const KpLevels lv,
                                                          const KgPlan* __restrict__ plan, const uint32_t* __restrict__ ghist2,
                                                          KpSel* __restrict__ st, int2* __restrict__ strip_cnt) {
  const int l = kp_level_at(lv.strip0, lv.n, blockIdx.x), first = kp_pick(lv.strip0, l);
  kp_count_strip(key2 + (size_t)first * kKpStrip, blockIdx.x - first, kp_pick(lv.W, l) * kp_pick(lv.H, l), plan[l].b,
                 ghist2 + l * 4 * kKpBins, st + 5 * l, strip_cnt + blockIdx.x);
}

__global__ __launch_bounds__(kKpScanThreads) void k_kpg_scan(const int2* __restrict__ strip_cnt, const KpLevels lv,
                                                             const KpSel* __restrict__ st, const KgPlan* __restrict__ plan,
                                                             const uint32_t* __restrict__ surv, const uint32_t* __restrict__ n_corners,
                                                             int2* __restrict__ strip_off, int32_t* __restrict__ level_row, int K,
                                                             gcs_keypoint_grid_outputs o) {
  __shared__ int n_all;
  const int t = threadIdx.x;
  kp_scan_strips(strip_cnt, lv.strip0[kKpMaxLevels], strip_off);
  if (t == 0) {
    int row = 0, survivors = 0, corners = 0;
#pragma unroll
    for (int l = 0; l < kKpMaxLevels; ++l) {
      int32_t c[6] = {0, 0, 0, l < lv.n ? lv.quota[l] : 0, 0, 0};
      if (l < lv.n && lv.strip0[l + 1] > lv.strip0[l]) {   // a level without pixels has no state and no plan
        const KgPlan p = plan[l];
        c[0] = kp_kept(st[5 * l + 4], p.b);
        c[1] = (int32_t)surv[l];
        c[2] = (int32_t)n_corners[l];
        c[4] = p.b;
        c[5] = p.t;
      }
      level_row[l] = row;
      for (int j = 0; j < 6; ++j) o.level_counts[6 * l + j] = c[j];
      row += c[0]; survivors += c[1]; corners += c[2];
    }
    o.counts[0] = row;
    o.counts[1] = survivors;
    o.counts[2] = corners;
    o.counts[3] = lv.n;
    n_all = row;
  }
  __syncthreads();
  for (int i = n_all + t; i < K; i += kKpScanThreads) {
    o.kp_u[i] = o.kp_v[i] = o.kp_response[i] = NAN;
    o.kp_level[i] = -1;
  }
}

__global__ __launch_bounds__(kKpThreads) void k_kpg_emit(const uint32_t* __restrict__ key, const uint32_t* __restrict__ key2,
                                                         const KpLevels lv, const KpSel* __restrict__ st,
                                                         const KgPlan* __restrict__ plan, const int2* __restrict__ strip_off,
                                                         const int32_t* __restrict__ level_row, int K, gcs_keypoint_grid_outputs o) {
  const int l = kp_level_at(lv.strip0, lv.n, blockIdx.x), first = kp_pick(lv.strip0, l);
  const int Wl = kp_pick(lv.W, l), Hl = kp_pick(lv.H, l);
  uint32_t kth;
  int need;
  kp_cut(st[5 * l + 4], plan[l].b, &kth, &need);
  const int2 mine = strip_off[blockIdx.x], head = strip_off[first];
  const KpPlace pl = {Wl, Hl, lv.W[0], lv.H[0], l, o.kp_level};
  const size_t off = (size_t)first * kKpStrip;
  kp_emit_strip<true>(key2 + off, blockIdx.x - first, Wl * Hl, kth, need, make_int2(mine.x - head.x, mine.y - head.y),
                      level_row[l], K, o.kp_u, o.kp_v, o.kp_response, pl, key + off);
}

// ---- checks and the host build

// (kp_check_config and kp_check_pyramid_config: gcs_keypoints_levels.h)

const char* kp_check_call(const gcs_keypoint_config& c, const gcs_keypoint_inputs* in, const gcs_keypoint_outputs* o) {
  if (!in || !o) return "null inputs or outputs";
  if (in->channels != 1 && in->channels != 3) return "channels is 1 (gray8) or 3 (rgb8)";
  if (in->width < 1 || in->height < 1 || in->width > c.max_width || in->height > c.max_height)
    return "width or height below 1 or above the context's capacity";
  if (in->pitch < (int64_t)in->channels * in->width) return "pitch below a row";
  if (!in->image || !o->kp_u || !o->kp_v || !o->kp_response || !o->counts) return "null array";
  return nullptr;
}

const char* kp_check_pyramid_call(const gcs_keypoint_pyramid_config& c, const gcs_keypoint_inputs* in,
                                  const gcs_keypoint_pyramid_outputs* o) {
  if (!in || !o) return "null inputs or outputs";
  if (in->channels != 1 && in->channels != 3) return "channels is 1 (gray8) or 3 (rgb8)";
  if (in->width < 1 || in->height < 1 || in->width > c.max_width || in->height > c.max_height)
    return "width or height below 1 or above the context's capacity";
  if (in->pitch < (int64_t)in->channels * in->width) return "pitch below a row";
  if (!in->image || !o->kp_u || !o->kp_v || !o->kp_response || !o->kp_level || !o->counts || !o->level_counts)
    return "null array";
  return nullptr;
}

// Steps 2-6 on a W x H grey image on the host: the kept pixels' raster indices and response bits in raster
// order; counts: n_keypoints, n_survivors, n_corners.  K = 0 keeps nothing.
void kp_host_level(const uint8_t* grey, int W, int H, int threshold, int edge, int K, double harris_k,
                   std::vector<int32_t>* kept_at, std::vector<uint32_t>* kept_bits, int32_t counts[3]) {
  const size_t n = (size_t)W * (size_t)H;
  std::vector<uint8_t> score(n, 0);
  int32_t n_corners = 0;
  for (int y = kKpFrame; y < H - kKpFrame; ++y)
    for (int x = kKpFrame; x < W - kKpFrame; ++x) {
      const int s = kp_fast_score(&grey[(size_t)y * W + x], W, threshold);
      score[(size_t)y * W + x] = (uint8_t)s;
      n_corners += s > 0;
    }
  std::vector<uint32_t> keys;   // the survivors, in raster order
  std::vector<int32_t> at;
  for (int y = edge; y < H - edge; ++y)
    for (int x = edge; x < W - edge; ++x) {
      const uint8_t* c = &score[(size_t)y * W + x];   // edge >= 4: the neighbours are inside
      const int s = c[0];
      if (!(s > 0 && s > c[-W - 1] && s > c[-W] && s > c[-W + 1] && s > c[-1] && s > c[1] && s > c[W - 1] && s > c[W] &&
            s > c[W + 1]))
        continue;
      int64_t a = 0, b = 0, cc = 0;
      for (int l = 0; l < kKpBlock * kKpBlock; ++l) {
        int ix, iy;
        kp_sobel(&grey[(size_t)(y + l / kKpBlock - kKpBlock / 2) * W + (x + l % kKpBlock - kKpBlock / 2)], W, &ix, &iy);
        a += ix * ix; b += iy * iy; cc += ix * iy;
      }
      float r = kp_response(a, b, cc, harris_k);
      uint32_t bits;
      memcpy(&bits, &r, 4);
      keys.push_back(kp_key_of_bits(bits));
      at.push_back(y * W + x);
    }
  const int total = (int)keys.size();
  uint32_t kth = K > 0 ? 0u : 0xffffffffu;   // (no finite response has the key 0xffffffff)
  int need = 0;
  if (K > 0 && total > K) {   // the K-th largest key; of the keys equal to it the first `need` in raster order stay
    std::vector<uint32_t> sorted(keys);
    std::nth_element(sorted.begin(), sorted.begin() + (K - 1), sorted.end(), std::greater<uint32_t>());
    kth = sorted[K - 1];
    int above = 0;
    for (uint32_t k : keys) above += k > kth;
    need = K - above;
  }
  int e = 0;
  for (int i = 0; i < total; ++i) {
    const bool tie = keys[i] == kth;
    if (keys[i] > kth || (tie && e < need)) {
      kept_at->push_back(at[i]);
      kept_bits->push_back(kp_bits_of_key(keys[i]));
    }
    e += tie;
  }
  counts[0] = (int32_t)kept_at->size();
  counts[1] = total;
  counts[2] = n_corners;
}

}  // namespace
}  // namespace gcs

using namespace gcs;

struct gcs_keypoint_ctx {
  gcs_keypoint_config cfg{};
  std::string err;
  int device = 0;
  hipStream_t stream = nullptr;   // the caller's (gcs_keypoint_ctx_set_stream); null: HIP's default stream
  void* d_mem = nullptr;
  size_t clear_bytes = 0;         // the histograms and n_corners, zeroed at the head of every call
  KpWork w{};
};

struct gcs_keypoint_pyramid_ctx {
  gcs_keypoint_pyramid_config cfg{};
  std::string err;
  int device = 0;
  hipStream_t stream = nullptr;
  void* d_mem = nullptr;
  size_t clear_bytes = 0;         // every level's histograms and n_corners, zeroed at the head of every call
  int cap_blocks = 0, cap_strips = 0;   // the packed workspace: 256-pixel blocks and 2048-key strips
  KpWork w{};                     // hist: per level 4 x 256 bins, then n_corners per level; st: per level [1..4]
  int32_t* level_row = nullptr;   // the first output row of every level
};

namespace {
int kpp_fail(gcs_keypoint_pyramid_ctx* c, int code, const std::string& m) {
  if (c) c->err = m;
  return code;
}
#define KPPCHK(ctx, expr)                                                                          \
  do {                                                                                            \
    hipError_t _e = (expr);                                                                       \
    if (_e != hipSuccess) return kpp_fail((ctx), GCS_ERR_HIP, std::string(#expr ": ") + hipGetErrorString(_e)); \
  } while (0)
int kp_fail(gcs_keypoint_ctx* c, int code, const std::string& m) {
  if (c) c->err = m;
  return code;
}
#define KPCHK(ctx, expr)                                                                          \
  do {                                                                                            \
    hipError_t _e = (expr);                                                                       \
    if (_e != hipSuccess) return kp_fail((ctx), GCS_ERR_HIP, std::string(#expr ": ") + hipGetErrorString(_e)); \
  } while (0)
}  // namespace

extern "C" {

int gcs_keypoint_config_defaults(gcs_keypoint_config* c) {
  if (!c) return GCS_ERR_ARG;
  memset(c, 0, sizeof(*c));
  c->fast_threshold = 20;
  c->edge_threshold = 31;
  c->max_keypoints = 4096;
  c->max_width = 1920;
  c->max_height = 1080;
  c->harris_k = 0.04;
  c->device = 0;
  return GCS_OK;
}

const char* gcs_keypoint_last_error(const gcs_keypoint_ctx* c) { return c ? c->err.c_str() : "null keypoint context"; }

int gcs_keypoint_ctx_destroy(gcs_keypoint_ctx* c) {
  if (!c) return GCS_OK;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  if (c->d_mem) (void)hipFree(c->d_mem);
  delete c;
  return GCS_OK;
}

int gcs_keypoint_ctx_create(const gcs_keypoint_config* cfg, gcs_keypoint_ctx** out) {
  if (!cfg || !out) return GCS_ERR_ARG;
  *out = nullptr;
  if (kp_check_config(cfg)) return GCS_ERR_ARG;
  auto* c = new gcs_keypoint_ctx();
  c->cfg = *cfg;
  c->device = cfg->device;
  const size_t px = (size_t)cfg->max_width * (size_t)cfg->max_height;
  const size_t strips = (px + kKpStrip - 1) / kKpStrip;
  auto up = [](size_t b) { return (b + 255) / 256 * 256; };
  const size_t z_hist = up(sizeof(uint32_t) * (4 * kKpBins + 1)), z_st = up(sizeof(KpSel) * 5);
  const size_t z_px = up(px), z_key = up(strips * kKpStrip * sizeof(uint32_t)), z_strip = up(strips * sizeof(int2));
  if (hipSetDevice(cfg->device) != hipSuccess ||
      hipMalloc(&c->d_mem, z_hist + z_st + 2 * z_px + z_key + 2 * z_strip) != hipSuccess) {
    gcs_keypoint_ctx_destroy(c);
    return GCS_ERR_HIP;
  }
  uint8_t* p = (uint8_t*)c->d_mem;
  c->w.hist = (uint32_t*)p; p += z_hist;
  c->w.st = (KpSel*)p; p += z_st;
  c->w.key = (uint32_t*)p; p += z_key;
  c->w.strip_cnt = (int2*)p; p += z_strip;
  c->w.strip_off = (int2*)p; p += z_strip;
  c->w.grey = p; p += z_px;
  c->w.score = p;
  c->clear_bytes = sizeof(uint32_t) * (4 * kKpBins + 1);
  *out = c;
  return GCS_OK;
}

int gcs_keypoint_ctx_set_stream(gcs_keypoint_ctx* c, void* stream) {
  if (!c) return GCS_ERR_ARG;
  hipStream_t ns = (hipStream_t)stream;
  if (ns == c->stream) return GCS_OK;
  KPCHK(c, hipSetDevice(c->device));
  KPCHK(c, hipStreamSynchronize(c->stream));  // the workspace is shared: the old stream's work completes first
  c->stream = ns;
  return GCS_OK;
}

int gcs_detect_keypoints_host(const gcs_keypoint_config* cfg, const gcs_keypoint_inputs* in, gcs_keypoint_outputs* out) {
  if (kp_check_config(cfg) || kp_check_call(*cfg, in, out)) return GCS_ERR_ARG;
  const int W = in->width, H = in->height, K = cfg->max_keypoints, edge = cfg->edge_threshold;
  const size_t n = (size_t)W * (size_t)H;
  std::vector<uint8_t> grey(n);
  for (int y = 0; y < H; ++y) {
    const uint8_t* row = in->image + (int64_t)y * in->pitch;
    for (int x = 0; x < W; ++x)
      grey[(size_t)y * W + x] = in->channels == 3 ? (uint8_t)kp_grey(row[3 * x], row[3 * x + 1], row[3 * x + 2]) : row[x];
  }
  std::vector<int32_t> at;
  std::vector<uint32_t> bits;
  int32_t counts[3];
  kp_host_level(grey.data(), W, H, cfg->fast_threshold, edge, K, cfg->harris_k, &at, &bits, counts);
  const int m = counts[0];
  for (int i = 0; i < m; ++i) {
    out->kp_u[i] = (float)(at[i] % W);
    out->kp_v[i] = (float)(at[i] / W);
    memcpy(&out->kp_response[i], &bits[i], 4);
  }
  for (int i = m; i < K; ++i) out->kp_u[i] = out->kp_v[i] = out->kp_response[i] = NAN;
  out->counts[0] = m;
  out->counts[1] = counts[1];
  out->counts[2] = counts[2];
  out->counts[3] = 0;
  return GCS_OK;
}

int gcs_detect_keypoints(gcs_keypoint_ctx* c, const gcs_keypoint_inputs* in, gcs_keypoint_outputs* out) {
  if (!c) return GCS_ERR_ARG;
  if (const char* m = kp_check_call(c->cfg, in, out)) return kp_fail(c, GCS_ERR_ARG, m);
  KPCHK(c, hipSetDevice(c->device));
  const int W = in->width, H = in->height, K = c->cfg.max_keypoints, n = W * H;
  const KpWork& w = c->w;
  uint32_t* n_corners = w.hist + 4 * kKpBins;
  KPCHK(c, hipMemsetAsync(w.hist, 0, c->clear_bytes, c->stream));
  const dim3 tiles((W + kKpTileW - 1) / kKpTileW, (H + kKpTileH - 1) / kKpTileH), threads(kKpThreads);
  if (in->channels == 3)
    hipLaunchKernelGGL(k_kp_score<3>, tiles, threads, 0, c->stream, in->image, in->pitch, W, H, c->cfg.fast_threshold,
                       w.grey, w.score, n_corners);
  else
    hipLaunchKernelGGL(k_kp_score<1>, tiles, threads, 0, c->stream, in->image, in->pitch, W, H, c->cfg.fast_threshold,
                       w.grey, w.score, n_corners);
  hipLaunchKernelGGL(k_kp_response, tiles, threads, 0, c->stream, w.score, w.grey, W, H, c->cfg.edge_threshold,
                     c->cfg.harris_k, w.key, w.hist);
  const int n_strips = (n + kKpStrip - 1) / kKpStrip;
  for (int pass = 1; pass <= 3; ++pass)
    hipLaunchKernelGGL(k_kp_hist, dim3(n_strips), threads, 0, c->stream, w.key, n, K, pass, w.hist, w.st);
  hipLaunchKernelGGL(k_kp_count, dim3(n_strips), threads, 0, c->stream, w.key, n, K, w.hist, w.st, w.strip_cnt);
  const gcs_keypoint_outputs o = *out;
  hipLaunchKernelGGL(k_kp_scan, dim3(1), dim3(kKpScanThreads), 0, c->stream, w.strip_cnt, n_strips, w.st, n_corners,
                     w.strip_off, K, o);
  hipLaunchKernelGGL(k_kp_emit, dim3(n_strips), threads, 0, c->stream, w.key, n, W, w.st, w.strip_off, K, o);
  KPCHK(c, hipGetLastError());
  return GCS_OK;
}

// ---- the pyramid

int gcs_keypoint_pyramid_config_defaults(gcs_keypoint_pyramid_config* c) {
  if (!c) return GCS_ERR_ARG;
  gcs_keypoint_config six;
  gcs_keypoint_config_defaults(&six);
  memset(c, 0, sizeof(*c));
  c->fast_threshold = six.fast_threshold;
  c->edge_threshold = six.edge_threshold;
  c->max_keypoints = six.max_keypoints;
  c->max_width = six.max_width;
  c->max_height = six.max_height;
  c->harris_k = six.harris_k;
  c->n_levels = 8;
  c->scale_num = 6;
  c->scale_den = 5;
  c->device = 0;
  return GCS_OK;
}

int gcs_keypoint_pyramid_layout(const gcs_keypoint_pyramid_config* cfg, int32_t width, int32_t height,
                                int32_t out[GCS_KEYPOINT_MAX_LEVELS][3]) {
  if (kp_check_pyramid_config(cfg) || !out || width < 1 || height < 1 || (int64_t)width * height > kKpMaxPixels)
    return GCS_ERR_ARG;
  const KpLevels lv = kp_levels(*cfg, width, height);
  for (int l = 0; l < kKpMaxLevels; ++l) {
    out[l][0] = lv.W[l];
    out[l][1] = lv.H[l];
    out[l][2] = lv.quota[l];
  }
  return GCS_OK;
}

const char* gcs_keypoint_pyramid_last_error(const gcs_keypoint_pyramid_ctx* c) {
  return c ? c->err.c_str() : "null keypoint pyramid context";
}

int gcs_keypoint_pyramid_ctx_destroy(gcs_keypoint_pyramid_ctx* c) {
  if (!c) return GCS_OK;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  if (c->d_mem) (void)hipFree(c->d_mem);
  delete c;
  return GCS_OK;
}

int gcs_keypoint_pyramid_ctx_create(const gcs_keypoint_pyramid_config* cfg, gcs_keypoint_pyramid_ctx** out) {
  if (!cfg || !out) return GCS_ERR_ARG;
  *out = nullptr;
  if (kp_check_pyramid_config(cfg)) return GCS_ERR_ARG;
  auto* c = new gcs_keypoint_pyramid_ctx();
  c->cfg = *cfg;
  c->device = cfg->device;
  // A level's size grows with the image's, so the table of max_width x max_height bounds every image's.
  const KpLevels cap = kp_levels(*cfg, cfg->max_width, cfg->max_height);
  c->cap_blocks = cap.block0[kKpMaxLevels];
  c->cap_strips = cap.strip0[kKpMaxLevels];
  const size_t px = (size_t)c->cap_blocks * kKpThreads, strips = (size_t)c->cap_strips;
  auto up = [](size_t b) { return (b + 255) / 256 * 256; };
  c->clear_bytes = sizeof(uint32_t) * (kKpMaxLevels * 4 * kKpBins + kKpMaxLevels);
  const size_t z_hist = up(c->clear_bytes), z_st = up(sizeof(KpSel) * 5 * kKpMaxLevels), z_row = up(sizeof(int32_t) * kKpMaxLevels);
  const size_t z_px = up(px), z_key = up(strips * kKpStrip * sizeof(uint32_t)), z_strip = up(strips * sizeof(int2));
  if (hipSetDevice(cfg->device) != hipSuccess ||
      hipMalloc(&c->d_mem, z_hist + z_st + z_row + 2 * z_px + z_key + 2 * z_strip) != hipSuccess) {
    gcs_keypoint_pyramid_ctx_destroy(c);
    return GCS_ERR_HIP;
  }
  uint8_t* p = (uint8_t*)c->d_mem;
  c->w.hist = (uint32_t*)p; p += z_hist;
  c->w.st = (KpSel*)p; p += z_st;
  c->level_row = (int32_t*)p; p += z_row;
  c->w.key = (uint32_t*)p; p += z_key;
  c->w.strip_cnt = (int2*)p; p += z_strip;
  c->w.strip_off = (int2*)p; p += z_strip;
  c->w.grey = p; p += z_px;
  c->w.score = p;
  *out = c;
  return GCS_OK;
}

int gcs_keypoint_pyramid_ctx_set_stream(gcs_keypoint_pyramid_ctx* c, void* stream) {
  if (!c) return GCS_ERR_ARG;
  hipStream_t ns = (hipStream_t)stream;
  if (ns == c->stream) return GCS_OK;
  KPPCHK(c, hipSetDevice(c->device));
  KPPCHK(c, hipStreamSynchronize(c->stream));  // the workspace is shared: the old stream's work completes first
  c->stream = ns;
  return GCS_OK;
}

int gcs_detect_keypoints_pyramid_host(const gcs_keypoint_pyramid_config* cfg, const gcs_keypoint_inputs* in,
                                      gcs_keypoint_pyramid_outputs* out) {
  if (kp_check_pyramid_config(cfg) || kp_check_pyramid_call(*cfg, in, out)) return GCS_ERR_ARG;
  const int W = in->width, H = in->height, K = cfg->max_keypoints;
  const KpLevels lv = kp_levels(*cfg, W, H);
  int32_t sum[3] = {0, 0, 0};
  int m = 0;
  std::vector<uint8_t> grey;
  for (int l = 0; l < kKpMaxLevels; ++l) {
    int32_t counts[3] = {0, 0, 0};
    if (lv.strip0[l + 1] > lv.strip0[l]) {   // the level has pixels
      const int Wl = lv.W[l], Hl = lv.H[l];
      grey.assign((size_t)Wl * Hl, 0);
      for (int y = 0; y < Hl; ++y)
        for (int x = 0; x < Wl; ++x) {
          int g;
          if (l == 0) {
            const uint8_t* p = in->image + (int64_t)y * in->pitch + (int64_t)in->channels * x;
            g = in->channels == 3 ? kp_grey(p[0], p[1], p[2]) : p[0];
          } else {
            g = in->channels == 3 ? kp_resample_pixel<3>(in->image, in->pitch, W, H, Wl, Hl, x, y)
                                  : kp_resample_pixel<1>(in->image, in->pitch, W, H, Wl, Hl, x, y);
          }
          grey[(size_t)y * Wl + x] = (uint8_t)g;
        }
      std::vector<int32_t> at;
      std::vector<uint32_t> bits;
      kp_host_level(grey.data(), Wl, Hl, cfg->fast_threshold, cfg->edge_threshold, lv.quota[l], cfg->harris_k, &at, &bits,
                    counts);
      for (size_t i = 0; i < at.size() && m < K; ++i, ++m) {   // (the quotas sum to K)
        out->kp_u[m] = kp_level0_coord(at[i] % Wl, W, Wl);
        out->kp_v[m] = kp_level0_coord(at[i] / Wl, H, Hl);
        memcpy(&out->kp_response[m], &bits[i], 4);
        out->kp_level[m] = l;
      }
    }
    for (int j = 0; j < 3; ++j) {
      out->level_counts[4 * l + j] = counts[j];
      sum[j] += counts[j];
    }
    out->level_counts[4 * l + 3] = l < lv.n ? lv.quota[l] : 0;
  }
  for (int i = m; i < K; ++i) {
    out->kp_u[i] = out->kp_v[i] = out->kp_response[i] = NAN;
    out->kp_level[i] = -1;
  }
  for (int j = 0; j < 3; ++j) out->counts[j] = sum[j];
  out->counts[3] = lv.n;
  return GCS_OK;
}

int gcs_detect_keypoints_pyramid(gcs_keypoint_pyramid_ctx* c, const gcs_keypoint_inputs* in,
                                 gcs_keypoint_pyramid_outputs* out) {
  if (!c) return GCS_ERR_ARG;
  if (const char* m = kp_check_pyramid_call(c->cfg, in, out)) return kpp_fail(c, GCS_ERR_ARG, m);
  const KpLevels lv = kp_levels(c->cfg, in->width, in->height);
  const int n_blocks = lv.block0[kKpMaxLevels], n_tiles = lv.tile0[kKpMaxLevels], n_strips = lv.strip0[kKpMaxLevels];
  if (n_blocks > c->cap_blocks || n_strips > c->cap_strips) return kpp_fail(c, GCS_ERR_ARG, "the image's levels exceed the workspace");
  KPPCHK(c, hipSetDevice(c->device));
  const int K = c->cfg.max_keypoints;
  const KpWork& w = c->w;
  uint32_t* n_corners = w.hist + kKpMaxLevels * 4 * kKpBins;
  KPPCHK(c, hipMemsetAsync(w.hist, 0, c->clear_bytes, c->stream));
  const dim3 threads(kKpThreads);
  if (in->channels == 3)
    hipLaunchKernelGGL(k_kpp_resample<3>, dim3(n_blocks), threads, 0, c->stream, in->image, in->pitch, lv, w.grey);
  else
    hipLaunchKernelGGL(k_kpp_resample<1>, dim3(n_blocks), threads, 0, c->stream, in->image, in->pitch, lv, w.grey);
  hipLaunchKernelGGL(k_kpp_score, dim3(n_tiles), threads, 0, c->stream, w.grey, lv, c->cfg.fast_threshold, w.score, n_corners);
  hipLaunchKernelGGL(k_kpp_response, dim3(n_tiles), threads, 0, c->stream, w.score, w.grey, lv, c->cfg.edge_threshold,
                     c->cfg.harris_k, w.key, w.hist);
  for (int pass = 1; pass <= 3; ++pass)
    hipLaunchKernelGGL(k_kpp_hist, dim3(n_strips), threads, 0, c->stream, w.key, lv, pass, w.hist, w.st);
  hipLaunchKernelGGL(k_kpp_count, dim3(n_strips), threads, 0, c->stream, w.key, lv, w.hist, w.st, w.strip_cnt);
  const gcs_keypoint_pyramid_outputs o = *out;
  hipLaunchKernelGGL(k_kpp_scan, dim3(1), dim3(kKpScanThreads), 0, c->stream, w.strip_cnt, lv, w.st, n_corners, w.strip_off,
                     c->level_row, K, o);
  hipLaunchKernelGGL(k_kpp_emit, dim3(n_strips), threads, 0, c->stream, w.key, lv, w.st, w.strip_off, c->level_row, K, o);
  KPPCHK(c, hipGetLastError());
  return GCS_OK;
}

}  // extern "C"

// ---- the grid of cells

struct gcs_keypoint_grid_ctx {
  gcs_keypoint_grid_config cfg{};
  std::string err;
  int device = 0;
  hipStream_t stream = nullptr;
  void* d_mem = nullptr;
  size_t clear_bytes = 0;         // both sets of histograms, n_corners, cells_with and the survivor counts
  int cap_blocks = 0, cap_strips = 0;
  KpWork w{};                     // as the pyramid's; hist: the response kernel's top-byte histograms
  uint32_t *key2 = nullptr, *hist2 = nullptr;   // the second key image (first the ranks) and its select's histograms
  uint32_t *n_corners = nullptr, *cells_with = nullptr, *surv = nullptr;   // per level: 1, 1024, 1
  KgPlan* plan = nullptr;         // per level
  int32_t* level_row = nullptr;
};

namespace {
int kpg_fail(gcs_keypoint_grid_ctx* c, int code, const std::string& m) {
  if (c) c->err = m;
  return code;
}
#define KPGCHK(ctx, expr)                                                                          \
  do {                                                                                            \
    hipError_t _e = (expr);                                                                       \
    if (_e != hipSuccess) return kpg_fail((ctx), GCS_ERR_HIP, std::string(#expr ": ") + hipGetErrorString(_e)); \
  } while (0)

gcs_keypoint_pyramid_config kg_pyramid_config(const gcs_keypoint_grid_config& c) {
  gcs_keypoint_pyramid_config p;
  memset(&p, 0, sizeof(p));
  p.fast_threshold = c.fast_threshold;
  p.edge_threshold = c.edge_threshold;
  p.max_keypoints = c.max_keypoints;
  p.max_width = c.max_width;
  p.max_height = c.max_height;
  p.harris_k = c.harris_k;
  p.n_levels = c.n_levels;
  p.scale_num = c.scale_num;
  p.scale_den = c.scale_den;
  p.device = c.device;
  return p;
}

const char* kg_check_config(const gcs_keypoint_grid_config* c) {
  if (!c) return "null config";
  const gcs_keypoint_pyramid_config ten = kg_pyramid_config(*c);
  if (const char* m = kp_check_pyramid_config(&ten)) return m;
  if (c->cell_size < kKgMinCell || c->cell_size > kKgMaxCell) return "cell_size outside [8, 64]";
  if (c->redistribute != 0 && c->redistribute != 1) return "redistribute is 0 or 1";
  return nullptr;
}

const char* kg_check_call(const gcs_keypoint_grid_config& c, const gcs_keypoint_inputs* in, const gcs_keypoint_grid_outputs* o) {
  if (!o) return "null inputs or outputs";
  const gcs_keypoint_pyramid_outputs six = {o->kp_u, o->kp_v, o->kp_response, o->kp_level, o->counts, o->level_counts};
  return kp_check_pyramid_call(kg_pyramid_config(c), in, &six);
}

// the cell table of a level table (a level's cells stay below 2^28 / 64, all of them below 2^31)
KgGrid kg_grid(const gcs_keypoint_grid_config& c, const KpLevels& lv, int32_t n_cy[kKpMaxLevels]) {
  KgGrid g{};
  g.cell = c.cell_size;
  g.edge = c.edge_threshold;
  g.redistribute = c.redistribute;
  for (int l = 0; l < kKpMaxLevels; ++l) {
    int nx = 0, ny = 0;
    if (lv.strip0[l + 1] > lv.strip0[l]) {
      nx = kg_cells(lv.W[l], c.edge_threshold, c.cell_size);
      ny = kg_cells(lv.H[l], c.edge_threshold, c.cell_size);
      if (nx == 0 || ny == 0) nx = ny = 0;
    }
    g.n_cx[l] = nx;
    n_cy[l] = ny;
    g.cell0[l + 1] = g.cell0[l] + nx * ny;
  }
  g.n_cells = g.cell0[kKpMaxLevels];
  return g;
}
}  // namespace

extern "C" {

int gcs_keypoint_grid_config_defaults(gcs_keypoint_grid_config* c) {
  if (!c) return GCS_ERR_ARG;
  gcs_keypoint_pyramid_config ten;
  gcs_keypoint_pyramid_config_defaults(&ten);
  memset(c, 0, sizeof(*c));
  c->fast_threshold = ten.fast_threshold;
  c->edge_threshold = ten.edge_threshold;
  c->max_keypoints = ten.max_keypoints;
  c->max_width = ten.max_width;
  c->max_height = ten.max_height;
  c->harris_k = ten.harris_k;
  c->n_levels = ten.n_levels;
  c->scale_num = ten.scale_num;
  c->scale_den = ten.scale_den;
  c->cell_size = 32;
  c->redistribute = 1;
  c->device = 0;
  return GCS_OK;
}

int gcs_keypoint_grid_layout(const gcs_keypoint_grid_config* cfg, int32_t width, int32_t height,
                             int32_t out[GCS_KEYPOINT_MAX_LEVELS][5]) {
  if (kg_check_config(cfg) || !out || width < 1 || height < 1 || (int64_t)width * height > kKpMaxPixels) return GCS_ERR_ARG;
  const KpLevels lv = kp_levels(kg_pyramid_config(*cfg), width, height);
  int32_t n_cy[kKpMaxLevels];
  const KgGrid g = kg_grid(*cfg, lv, n_cy);
  for (int l = 0; l < kKpMaxLevels; ++l) {
    out[l][0] = lv.W[l];
    out[l][1] = lv.H[l];
    out[l][2] = lv.quota[l];
    out[l][3] = g.n_cx[l];
    out[l][4] = n_cy[l];
  }
  return GCS_OK;
}

const char* gcs_keypoint_grid_last_error(const gcs_keypoint_grid_ctx* c) {
  return c ? c->err.c_str() : "null keypoint grid context";
}

int gcs_keypoint_grid_ctx_destroy(gcs_keypoint_grid_ctx* c) {
  if (!c) return GCS_OK;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  if (c->d_mem) (void)hipFree(c->d_mem);
  delete c;
  return GCS_OK;
}

int gcs_keypoint_grid_ctx_create(const gcs_keypoint_grid_config* cfg, gcs_keypoint_grid_ctx** out) {
  if (!cfg || !out) return GCS_ERR_ARG;
  *out = nullptr;
  if (kg_check_config(cfg)) return GCS_ERR_ARG;
  auto* c = new gcs_keypoint_grid_ctx();
  c->cfg = *cfg;
  c->device = cfg->device;
  const KpLevels cap = kp_levels(kg_pyramid_config(*cfg), cfg->max_width, cfg->max_height);
  c->cap_blocks = cap.block0[kKpMaxLevels];
  c->cap_strips = cap.strip0[kKpMaxLevels];
  const size_t px = (size_t)c->cap_blocks * kKpThreads, strips = (size_t)c->cap_strips;
  auto up = [](size_t b) { return (b + 255) / 256 * 256; };
  const size_t n_hist = (size_t)kKpMaxLevels * 4 * kKpBins, n_with = (size_t)kKpMaxLevels * kKgMaxPerCell;
  c->clear_bytes = sizeof(uint32_t) * (2 * n_hist + n_with + 2 * kKpMaxLevels);
  const size_t z_clear = up(c->clear_bytes), z_st = up(sizeof(KpSel) * 5 * kKpMaxLevels), z_row = up(sizeof(int32_t) * kKpMaxLevels);
  const size_t z_plan = up(sizeof(KgPlan) * kKpMaxLevels);
  const size_t z_px = up(px), z_key = up(strips * kKpStrip * sizeof(uint32_t)), z_strip = up(strips * sizeof(int2));
  if (hipSetDevice(cfg->device) != hipSuccess ||
      hipMalloc(&c->d_mem, z_clear + z_st + z_row + z_plan + 2 * z_px + 2 * z_key + 2 * z_strip) != hipSuccess) {
    gcs_keypoint_grid_ctx_destroy(c);
    return GCS_ERR_HIP;
  }
  uint8_t* p = (uint8_t*)c->d_mem;
  c->w.hist = (uint32_t*)p;
  c->hist2 = c->w.hist + n_hist;
  c->cells_with = c->hist2 + n_hist;   // (a multiple of 16 bytes from the allocation's start: read as uint4)
  c->n_corners = c->cells_with + n_with;
  c->surv = c->n_corners + kKpMaxLevels;
  p += z_clear;
  c->w.st = (KpSel*)p; p += z_st;
  c->level_row = (int32_t*)p; p += z_row;
  c->plan = (KgPlan*)p; p += z_plan;
  c->w.key = (uint32_t*)p; p += z_key;
  c->key2 = (uint32_t*)p; p += z_key;
  c->w.strip_cnt = (int2*)p; p += z_strip;
  c->w.strip_off = (int2*)p; p += z_strip;
  c->w.grey = p; p += z_px;
  c->w.score = p;
  *out = c;
  return GCS_OK;
}

int gcs_keypoint_grid_ctx_set_stream(gcs_keypoint_grid_ctx* c, void* stream) {
  if (!c) return GCS_ERR_ARG;
  hipStream_t ns = (hipStream_t)stream;
  if (ns == c->stream) return GCS_OK;
  KPGCHK(c, hipSetDevice(c->device));
  KPGCHK(c, hipStreamSynchronize(c->stream));  // the workspace is shared: the old stream's work completes first
  c->stream = ns;
  return GCS_OK;
}

int gcs_detect_keypoints_grid_host(const gcs_keypoint_grid_config* cfg, const gcs_keypoint_inputs* in,
                                   gcs_keypoint_grid_outputs* out) {
  if (kg_check_config(cfg) || kg_check_call(*cfg, in, out)) return GCS_ERR_ARG;
  const int W = in->width, H = in->height, K = cfg->max_keypoints, e = cfg->edge_threshold, cs = cfg->cell_size;
  const KpLevels lv = kp_levels(kg_pyramid_config(*cfg), W, H);
  int32_t n_cy[kKpMaxLevels];
  const KgGrid gr = kg_grid(*cfg, lv, n_cy);
  // every level's survivors in raster order: raster index and the response's key
  std::vector<int32_t> at[kKpMaxLevels];
  std::vector<uint32_t> key[kKpMaxLevels];
  int32_t surv[kKpMaxLevels] = {}, corners[kKpMaxLevels] = {}, budget[kKpMaxLevels];
  std::vector<uint8_t> grey;
  for (int l = 0; l < kKpMaxLevels; ++l) {
    if (lv.strip0[l + 1] == lv.strip0[l]) continue;   // the level has no pixels
    const int Wl = lv.W[l], Hl = lv.H[l];
    grey.assign((size_t)Wl * Hl, 0);
    for (int y = 0; y < Hl; ++y)
      for (int x = 0; x < Wl; ++x) {
        int g;
        if (l == 0) {
          const uint8_t* p = in->image + (int64_t)y * in->pitch + (int64_t)in->channels * x;
          g = in->channels == 3 ? kp_grey(p[0], p[1], p[2]) : p[0];
        } else {
          g = in->channels == 3 ? kp_resample_pixel<3>(in->image, in->pitch, W, H, Wl, Hl, x, y)
                                : kp_resample_pixel<1>(in->image, in->pitch, W, H, Wl, Hl, x, y);
        }
        grey[(size_t)y * Wl + x] = (uint8_t)g;
      }
    std::vector<uint32_t> bits;
    int32_t counts[3];
    // (a cap no level reaches: every survivor comes back)
    kp_host_level(grey.data(), Wl, Hl, cfg->fast_threshold, e, INT32_MAX, cfg->harris_k, &at[l], &bits, counts);
    key[l].resize(bits.size());
    for (size_t i = 0; i < bits.size(); ++i) key[l][i] = kp_key_of_bits(bits[i]);
    surv[l] = counts[1];
    corners[l] = counts[2];
  }
  kg_budgets(lv.quota, surv, cfg->redistribute, budget);
  int32_t sum[3] = {0, 0, 0};
  int m = 0;
  for (int l = 0; l < kKpMaxLevels; ++l) {
    const int Wl = lv.W[l], Hl = lv.H[l], n = (int)at[l].size(), b = budget[l];
    int t = 0, kept = 0;
    if (n) {
      // G3: the survivors by (cell, key descending, raster ascending); a survivor's rank is its place in its cell
      const int ncx = gr.n_cx[l];
      std::vector<int32_t> cell(n), order(n), rank(n);
      for (int i = 0; i < n; ++i) {
        cell[i] = ((at[l][i] / Wl - e) / cs) * ncx + (at[l][i] % Wl - e) / cs;
        order[i] = i;
      }
      const std::vector<uint32_t>& k = key[l];
      std::sort(order.begin(), order.end(), [&](int32_t a, int32_t c2) {
        if (cell[a] != cell[c2]) return cell[a] < cell[c2];
        if (k[a] != k[c2]) return k[a] > k[c2];
        return a < c2;   // (the list is in raster order)
      });
      std::vector<int32_t> cells_with(kKgMaxPerCell, 0);
      for (int i = 0, r = 0; i < n; ++i) {
        r = (i && cell[order[i]] == cell[order[i - 1]]) ? r + 1 : 1;
        rank[order[i]] = r;
        if (i + 1 == n || cell[order[i + 1]] != cell[order[i]]) ++cells_with[r - 1];
      }
      int64_t at_t;
      t = kg_cap_host(cells_with.data(), b, &at_t);
      const int rem = (int)(b - at_t);
      // the remainder: the rem best of rank t + 1 by (key descending, raster ascending)
      std::vector<int32_t> next;
      for (int i = 0; i < n; ++i)
        if (rank[i] == t + 1) next.push_back(i);
      std::sort(next.begin(), next.end(), [&](int32_t a, int32_t c2) { return k[a] != k[c2] ? k[a] > k[c2] : a < c2; });
      std::vector<uint8_t> keep(n, 0);
      for (int i = 0; i < n; ++i) keep[i] = rank[i] <= t;
      for (int i = 0; i < rem && i < (int)next.size(); ++i) keep[next[i]] = 1;
      for (int i = 0; i < n; ++i) {
        if (!keep[i]) continue;
        ++kept;
        if (m >= K) continue;   // (the budgets sum to at most K)
        out->kp_u[m] = kp_level0_coord(at[l][i] % Wl, W, Wl);
        out->kp_v[m] = kp_level0_coord(at[l][i] / Wl, H, Hl);
        const uint32_t bits = kp_bits_of_key(k[i]);
        memcpy(&out->kp_response[m], &bits, 4);
        out->kp_level[m] = l;
        ++m;
      }
    }
    const int32_t row[6] = {kept, surv[l], corners[l], l < lv.n ? lv.quota[l] : 0, b, t};
    for (int j = 0; j < 6; ++j) out->level_counts[6 * l + j] = row[j];
    for (int j = 0; j < 3; ++j) sum[j] += row[j];
  }
  for (int i = m; i < K; ++i) {
    out->kp_u[i] = out->kp_v[i] = out->kp_response[i] = NAN;
    out->kp_level[i] = -1;
  }
  for (int j = 0; j < 3; ++j) out->counts[j] = sum[j];
  out->counts[3] = lv.n;
  return GCS_OK;
}

int gcs_detect_keypoints_grid(gcs_keypoint_grid_ctx* c, const gcs_keypoint_inputs* in, gcs_keypoint_grid_outputs* out) {
  if (!c) return GCS_ERR_ARG;
  if (const char* m = kg_check_call(c->cfg, in, out)) return kpg_fail(c, GCS_ERR_ARG, m);
  const KpLevels lv = kp_levels(kg_pyramid_config(c->cfg), in->width, in->height);
  const int n_blocks = lv.block0[kKpMaxLevels], n_tiles = lv.tile0[kKpMaxLevels], n_strips = lv.strip0[kKpMaxLevels];
  if (n_blocks > c->cap_blocks || n_strips > c->cap_strips) return kpg_fail(c, GCS_ERR_ARG, "the image's levels exceed the workspace");
  int32_t n_cy[kKpMaxLevels];
  const KgGrid gr = kg_grid(c->cfg, lv, n_cy);
  KPGCHK(c, hipSetDevice(c->device));
  const int K = c->cfg.max_keypoints;
  const KpWork& w = c->w;
  KPGCHK(c, hipMemsetAsync(w.hist, 0, c->clear_bytes, c->stream));
  const dim3 threads(kKpThreads);
  if (in->channels == 3)
    hipLaunchKernelGGL(k_kpp_resample<3>, dim3(n_blocks), threads, 0, c->stream, in->image, in->pitch, lv, w.grey);
  else
    hipLaunchKernelGGL(k_kpp_resample<1>, dim3(n_blocks), threads, 0, c->stream, in->image, in->pitch, lv, w.grey);
  hipLaunchKernelGGL(k_kpp_score, dim3(n_tiles), threads, 0, c->stream, w.grey, lv, c->cfg.fast_threshold, w.score, c->n_corners);
  hipLaunchKernelGGL(k_kpp_response, dim3(n_tiles), threads, 0, c->stream, w.score, w.grey, lv, c->cfg.edge_threshold,
                     c->cfg.harris_k, w.key, w.hist);
  hipLaunchKernelGGL(k_kpg_rank, dim3(std::max(gr.n_cells, 1)), threads, 0, c->stream, w.key, lv, gr, c->key2, c->cells_with,
                     c->surv);
  hipLaunchKernelGGL(k_kpg_plan, dim3(kKpMaxLevels), threads, 0, c->stream, lv, gr.redistribute, c->surv, c->cells_with,
                     c->plan);
  hipLaunchKernelGGL(k_kpg_mark, dim3(n_strips), threads, 0, c->stream, w.key, c->key2, lv, c->plan, c->hist2);
  for (int pass = 1; pass <= 3; ++pass)
    hipLaunchKernelGGL(k_kpg_hist, dim3(n_strips), threads, 0, c->stream, c->key2, lv, pass, c->plan, c->hist2, w.st);
  hipLaunchKernelGGL(k_kpg_count, dim3(n_strips), threads, 0, c->stream, c->key2, lv, c->plan, c->hist2, w.st, w.strip_cnt);
  const gcs_keypoint_grid_outputs o = *out;
  hipLaunchKernelGGL(k_kpg_scan, dim3(1), dim3(kKpScanThreads), 0, c->stream, w.strip_cnt, lv, w.st, c->plan, c->surv,
                     c->n_corners, w.strip_off, c->level_row, K, o);
  hipLaunchKernelGGL(k_kpg_emit, dim3(n_strips), threads, 0, c->stream, w.key, c->key2, lv, w.st, c->plan, w.strip_off,
                     c->level_row, K, o);
  KPGCHK(c, hipGetLastError());
  return GCS_OK;
}

}  // extern "C"
