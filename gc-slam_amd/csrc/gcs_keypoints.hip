// Keypoints on the GPU: the detector front of the FAST / ORB recipe at pyramid level 0, from an 8-bit image to
// the (kp_u, kp_v, kp_response) arrays gcs_visfeat_inputs reads.  The project's own definition
// (include/gcslam_hip.h): no pyramid, no orientation, no descriptors, and no parity with cv::ORB.  Kernels:
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

#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <functional>
#include <string>
#include <vector>

#include "gcs_keypoints_math.h"
#include "gcslam_hip.h"

#pragma clang fp contract(off)

namespace gcs {
namespace {

constexpr int kKpTileW = 64, kKpTileH = 16, kKpThreads = 256;
constexpr int kKpRows = kKpTileH / (kKpThreads / kKpTileW);   // pixels per thread, one per 4 rows
constexpr int kKpGW = kKpTileW + 2 * kKpFrame, kKpGH = kKpTileH + 2 * kKpFrame, kKpGStride = 72;
constexpr int kKpRawDw = 56;       // dwords per staged row: 3 * 70 bytes and up to 3 in front of them, 54 dwords
constexpr int kKpSW = kKpTileW + 2, kKpSH = kKpTileH + 2, kKpSStride = 68;
constexpr int kKpStrip = 2048, kKpPerThread = kKpStrip / kKpThreads;
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

template <int CH>
__global__ __launch_bounds__(kKpThreads) void k_kp_score(const uint8_t* __restrict__ img, int64_t pitch, int W, int H,
                                                         int threshold, uint8_t* __restrict__ grey_out,
                                                         uint8_t* __restrict__ score_out, uint32_t* __restrict__ n_corners) {
  __shared__ uint32_t raw[kKpGH * kKpRawDw];
  __shared__ uint8_t grey[kKpGH * kKpGStride];
  const int t = threadIdx.x;
  const int x0 = blockIdx.x * kKpTileW, y0 = blockIdx.y * kKpTileH;
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
      grey_out[y * W + x] = c[0];
      score_out[y * W + x] = (uint8_t)s;
      corners += s > 0;
    }
  }
  for (int off = 32; off > 0; off >>= 1) corners += __shfl_xor(corners, off, 64);
  if ((t & 63) == 0 && corners) atomicAdd(n_corners, (uint32_t)corners);
}

// ---- k_kp_response

__global__ __launch_bounds__(kKpThreads) void k_kp_response(const uint8_t* __restrict__ score, const uint8_t* __restrict__ grey,
                                                            int W, int H, int edge, double harris_k,
                                                            uint32_t* __restrict__ key, uint32_t* __restrict__ ghist) {
  __shared__ uint8_t sc[kKpSH * kKpSStride];
  __shared__ int list[kKpTileW * kKpTileH];
  __shared__ int n_list;
  __shared__ uint32_t hist[kKpBins];
  const int t = threadIdx.x;
  const int x0 = blockIdx.x * kKpTileW, y0 = blockIdx.y * kKpTileH;
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

// a thread's keys of its strip: [blockIdx.x * 2048 + 8 t, + 8), zeros beyond n (the allocation is whole strips)
__device__ inline int kp_load_keys(const uint32_t* __restrict__ key, int n, uint32_t* k) {
  const int i0 = blockIdx.x * kKpStrip + threadIdx.x * kKpPerThread;
  const uint4 lo = *(const uint4*)(key + i0), hi = *(const uint4*)(key + i0 + 4);
  const uint32_t v[kKpPerThread] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
  for (int j = 0; j < kKpPerThread; ++j) k[j] = i0 + j < n ? v[j] : 0u;
  return i0;
}

__global__ __launch_bounds__(kKpThreads) void k_kp_hist(const uint32_t* __restrict__ key, int n, int K, int pass,
                                                        uint32_t* __restrict__ ghist, KpSel* __restrict__ st) {
  __shared__ uint32_t s[kKpBins];
  __shared__ KpSel box;
  const int t = threadIdx.x;
  const KpSel first = {0u, K, 0, 0};
  const KpSel cur = kp_resolve(ghist + (pass - 1) * kKpBins, pass == 1 ? first : st[pass - 1], pass - 1, s, &box);
  if (blockIdx.x == 0 && t == 0) st[pass] = cur;
  if (cur.all) return;
  s[t] = 0;
  __syncthreads();
  uint32_t k[kKpPerThread];
  kp_load_keys(key, n, k);
  const int shift = 32 - 8 * pass;
#pragma unroll
  for (int j = 0; j < kKpPerThread; ++j)   // (a key of 0 shares no chosen byte: the top byte of a real key is never 0)
    if (k[j] && (k[j] >> shift) == (cur.prefix >> shift)) atomicAdd(&s[(k[j] >> (shift - 8)) & 255u], 1u);
  __syncthreads();
  if (s[t]) atomicAdd(&ghist[pass * kKpBins + t], s[t]);
}

__device__ inline int kp_wave_incl(int x) {
  const int lane = threadIdx.x & 63;
  for (int off = 1; off < 64; off <<= 1) {
    const int y = __shfl_up(x, off, 64);
    if (lane >= off) x += y;
  }
  return x;
}

__global__ __launch_bounds__(kKpThreads) void k_kp_count(const uint32_t* __restrict__ key, int n, const uint32_t* __restrict__ ghist,
                                                         KpSel* __restrict__ st, int2* __restrict__ strip_cnt) {
  __shared__ uint32_t s[kKpBins];
  __shared__ KpSel box;
  __shared__ int2 part[kKpThreads / 64];
  const int t = threadIdx.x;
  const KpSel cur = kp_resolve(ghist + 3 * kKpBins, st[3], 3, s, &box);
  if (blockIdx.x == 0 && t == 0) st[4] = cur;
  const uint32_t kth = cur.all ? 0u : cur.prefix;
  uint32_t k[kKpPerThread];
  kp_load_keys(key, n, k);
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
    strip_cnt[blockIdx.x] = c;
  }
}

__global__ __launch_bounds__(kKpScanThreads) void k_kp_scan(const int2* __restrict__ strip_cnt, int n_strips,
                                                            const KpSel* __restrict__ st, const uint32_t* __restrict__ n_corners,
                                                            int2* __restrict__ strip_off, int K, gcs_keypoint_outputs o) {
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

__global__ __launch_bounds__(kKpThreads) void k_kp_emit(const uint32_t* __restrict__ key, int n, int W,
                                                        const KpSel* __restrict__ st, const int2* __restrict__ strip_off,
                                                        int K, gcs_keypoint_outputs o) {
  __shared__ int2 part[kKpThreads / 64];
  const int t = threadIdx.x;
  const KpSel cur = st[4];
  const uint32_t kth = cur.all ? 0u : cur.prefix;
  const int need = cur.all ? 0 : cur.rem;   // of the keys equal to kth, the first `need` in raster order are kept
  uint32_t k[kKpPerThread];
  const int i0 = kp_load_keys(key, n, k);
  int gt = 0, eq = 0;
#pragma unroll
  for (int j = 0; j < kKpPerThread; ++j) {
    gt += k[j] > kth;
    eq += k[j] == kth;
  }
  const int ig = kp_wave_incl(gt), ie = kp_wave_incl(eq);
  if ((t & 63) == 63) part[t >> 6] = make_int2(ig, ie);
  __syncthreads();
  int2 base = strip_off[blockIdx.x];
  for (int w = 0; w < (t >> 6); ++w) { base.x += part[w].x; base.y += part[w].y; }
  int g = base.x + ig - gt, e = base.y + ie - eq;   // keys above / equal to kth before this thread's, in raster order
#pragma unroll
  for (int j = 0; j < kKpPerThread; ++j) {
    const bool above = k[j] > kth, tie = k[j] == kth;
    if (above || (tie && e < need)) {
      const int pos = g + min(e, need), i = i0 + j;
      if (pos < K) {
        o.kp_u[pos] = (float)(i % W);
        o.kp_v[pos] = (float)(i / W);
        o.kp_response[pos] = __uint_as_float(kp_bits_of_key(k[j]));
      }
    }
    g += above;
    e += tie;
  }
}

// ---- checks and the host build

const char* kp_check_config(const gcs_keypoint_config* c) {
  if (!c) return "null config";
  if (c->fast_threshold < 0 || c->fast_threshold > 255) return "fast_threshold outside [0, 255]";
  if (c->edge_threshold < kKpMinEdge) return "edge_threshold below 4";
  if (c->max_keypoints < 1 || c->max_keypoints > kKpMaxKeypoints) return "max_keypoints outside [1, 65536]";
  if (c->max_width < 1 || c->max_height < 1 || (int64_t)c->max_width * c->max_height > kKpMaxPixels)
    return "max_width or max_height below 1, or more than 2^28 pixels";
  if (!std::isfinite(c->harris_k)) return "harris_k not finite";
  return nullptr;
}

const char* kp_check_call(const gcs_keypoint_config& c, const gcs_keypoint_inputs* in, const gcs_keypoint_outputs* o) {
  if (!in || !o) return "null inputs or outputs";
  if (in->channels != 1 && in->channels != 3) return "channels is 1 (gray8) or 3 (rgb8)";
  if (in->width < 1 || in->height < 1 || in->width > c.max_width || in->height > c.max_height)
    return "width or height below 1 or above the context's capacity";
  if (in->pitch < (int64_t)in->channels * in->width) return "pitch below a row";
  if (!in->image || !o->kp_u || !o->kp_v || !o->kp_response || !o->counts) return "null array";
  return nullptr;
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

namespace {
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
  std::vector<uint8_t> grey(n), score(n, 0);
  for (int y = 0; y < H; ++y) {
    const uint8_t* row = in->image + (int64_t)y * in->pitch;
    for (int x = 0; x < W; ++x)
      grey[(size_t)y * W + x] = in->channels == 3 ? (uint8_t)kp_grey(row[3 * x], row[3 * x + 1], row[3 * x + 2]) : row[x];
  }
  int32_t n_corners = 0;
  for (int y = kKpFrame; y < H - kKpFrame; ++y)
    for (int x = kKpFrame; x < W - kKpFrame; ++x) {
      const int s = kp_fast_score(&grey[(size_t)y * W + x], W, cfg->fast_threshold);
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
      float r = kp_response(a, b, cc, cfg->harris_k);
      uint32_t bits;
      memcpy(&bits, &r, 4);
      keys.push_back(kp_key_of_bits(bits));
      at.push_back(y * W + x);
    }
  const int total = (int)keys.size();
  uint32_t kth = 0;
  int need = 0;
  if (total > K) {   // the K-th largest key; of the keys equal to it the first `need` in raster order stay
    std::vector<uint32_t> sorted(keys);
    std::nth_element(sorted.begin(), sorted.begin() + (K - 1), sorted.end(), std::greater<uint32_t>());
    kth = sorted[K - 1];
    int above = 0;
    for (uint32_t k : keys) above += k > kth;
    need = K - above;
  }
  int m = 0, e = 0;
  for (int i = 0; i < total; ++i) {
    const bool tie = keys[i] == kth;
    if (keys[i] > kth || (tie && e < need)) {
      const uint32_t bits = kp_bits_of_key(keys[i]);
      out->kp_u[m] = (float)(at[i] % W);
      out->kp_v[m] = (float)(at[i] / W);
      memcpy(&out->kp_response[m], &bits, 4);
      ++m;
    }
    e += tie;
  }
  for (int i = m; i < K; ++i) out->kp_u[i] = out->kp_v[i] = out->kp_response[i] = NAN;
  out->counts[0] = m;
  out->counts[1] = total;
  out->counts[2] = n_corners;
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
  hipLaunchKernelGGL(k_kp_count, dim3(n_strips), threads, 0, c->stream, w.key, n, w.hist, w.st, w.strip_cnt);
  const gcs_keypoint_outputs o = *out;
  hipLaunchKernelGGL(k_kp_scan, dim3(1), dim3(kKpScanThreads), 0, c->stream, w.strip_cnt, n_strips, w.st, n_corners,
                     w.strip_off, K, o);
  hipLaunchKernelGGL(k_kp_emit, dim3(n_strips), threads, 0, c->stream, w.key, n, W, w.st, w.strip_off, K, o);
  KPCHK(c, hipGetLastError());
  return GCS_OK;
}

}  // extern "C"
