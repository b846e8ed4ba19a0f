// Bounds check of the keypoint detector's border / halo arithmetic on the host: gcs_detect_keypoints_host over
// the edge shapes, every image in a heap block of exactly (H - 1) * pitch + W * channels bytes and every
// output array of exactly max_keypoints values, so that a read or write one byte outside is an error under
// AddressSanitizer.  Built with -fsanitize=address,undefined for the host and run on the CPU only:
//   make -C gc-slam_amd keypoints_host_check && tools/keypoints_host_check
// Exit code 0: every call returned GCS_OK with the counts the shape implies.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <cmath>
#include <vector>

#include "gcslam_hip.h"

namespace {

uint32_t g_state = 12345u;
uint8_t next_byte() {   // a small LCG: the same images every run
  g_state = g_state * 1664525u + 1013904223u;
  return (uint8_t)(g_state >> 24);
}

struct Result {
  int rc;
  int32_t counts[4];
  float u0, v0;
};

// mode 0: noise, 1: zeros with 255 at the centre
Result run(int W, int H, int ch, int pad, int edge, int mode, int cap = 64) {
  gcs_keypoint_config cfg;
  gcs_keypoint_config_defaults(&cfg);
  cfg.edge_threshold = edge;
  cfg.max_keypoints = cap;
  cfg.max_width = W;
  cfg.max_height = H;
  const int64_t pitch = (int64_t)W * ch + pad;
  const size_t bytes = (size_t)(H - 1) * (size_t)pitch + (size_t)W * ch;
  uint8_t* img = (uint8_t*)malloc(bytes);
  for (size_t i = 0; i < bytes; ++i) img[i] = 0xAA;   // between the rows
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W * ch; ++x) img[(size_t)y * pitch + x] = mode == 0 ? next_byte() : 0;
  if (mode == 1)
    for (int c = 0; c < ch; ++c) img[(size_t)(H / 2) * pitch + (size_t)(W / 2) * ch + c] = 255;
  float* u = (float*)malloc(sizeof(float) * cap);
  float* v = (float*)malloc(sizeof(float) * cap);
  float* r = (float*)malloc(sizeof(float) * cap);
  int32_t* counts = (int32_t*)malloc(sizeof(int32_t) * 4);
  gcs_keypoint_inputs in = {img, ch, pitch, W, H};
  gcs_keypoint_outputs out = {u, v, r, counts};
  Result res{};
  res.rc = gcs_detect_keypoints_host(&cfg, &in, &out);
  for (int i = 0; i < 4; ++i) res.counts[i] = counts[i];
  res.u0 = u[0];
  res.v0 = v[0];
  if (res.rc == GCS_OK)
    for (int i = counts[0]; i < cap; ++i)
      if (!std::isnan(u[i]) || !std::isnan(v[i]) || !std::isnan(r[i])) res.rc = -100;   // the padding is NaN
  free(img); free(u); free(v); free(r); free(counts);
  return res;
}

int g_failed = 0;
void expect(const char* what, const Result& r, bool ok) {
  printf("%-28s rc %d  counts %d %d %d %d  %s\n", what, r.rc, r.counts[0], r.counts[1], r.counts[2], r.counts[3],
         ok ? "ok" : "UNEXPECTED");
  if (!ok) ++g_failed;
}

}  // namespace

int main() {
  char name[64];
  for (int ch = 1; ch <= 3; ch += 2) {
    Result r = run(1, 1, ch, 0, 4, 0);
    expect(ch == 1 ? "1x1 gray8" : "1x1 rgb8", r, r.rc == 0 && r.counts[0] == 0 && r.counts[2] == 0);
    r = run(6, 6, ch, 0, 4, 0);
    expect("tiny 6x6", r, r.rc == 0 && r.counts[0] == 0 && r.counts[2] == 0);
    r = run(7, 200, ch, 0, 4, 0);
    expect("tiny 7x200", r, r.rc == 0 && r.counts[0] == 0);
    r = run(200, 8, ch, 0, 4, 0);
    expect("tiny 200x8", r, r.rc == 0 && r.counts[0] == 0);
    r = run(64, 48, ch, 0, 31, 0);
    expect("tiny 64x48 edge 31", r, r.rc == 0 && r.counts[0] == 0 && r.counts[2] > 0);
    r = run(9, 9, ch, 0, 4, 1);
    expect("dot 9x9", r, r.rc == 0 && r.counts[0] == 1 && r.counts[1] == 1 && r.counts[2] == 1 && r.u0 == 4.0f && r.v0 == 4.0f);
    for (int pad = 1; pad <= 13; pad += 6) {
      snprintf(name, sizeof(name), "61x47 pitch + %d", pad);
      const uint32_t seed = g_state;
      const Result packed = run(61, 47, ch, 0, 4, 0);
      g_state = seed;   // the same pixels again, rows further apart
      r = run(61, 47, ch, pad, 4, 0);
      expect(name, r, r.rc == 0 && r.counts[0] > 0 && r.counts[0] == packed.counts[0] && r.counts[2] == packed.counts[2]);
    }
    for (int n = 7; n <= 12; ++n) {
      snprintf(name, sizeof(name), "%dx%d edge 4", n, n);
      r = run(n, n, ch, 0, 4, 0);
      expect(name, r, r.rc == 0 && (n >= 9 || r.counts[0] == 0));
      snprintf(name, sizeof(name), "%dx%d edge 4 dot, cap 1", n, n);
      r = run(n, n, ch, 3, 4, 1, 1);
      expect(name, r, r.rc == 0 && r.counts[0] == (n >= 9 ? 1 : 0) && r.counts[2] == 1);
    }
  }
  printf(g_failed ? "%d unexpected\n" : "all as expected\n", g_failed);
  return g_failed ? 1 : 0;
}
