// A fixed-size point cloud from a depth map (include/hifihr.h "Depth map to points": hifihr_depth_points), the reference's
// utils/fh_utils.py batch_depth2pc as ONE launch: P draws, uniform and with replacement, among the valid pixels of each sample, each
// back-projected through the inverse of the sample's 3 x 3 intrinsics.
//
// One workgroup per sample.  Every wave turns 64 pixels at a time into a validity word with __ballot; the words and their exclusive
// prefix counts stay in LDS (H W <= 512 x 512: 4096 words, 32 KB + 16 KB).  The prefix is one scan in a fixed order (integers: the same on
// every call).  Then every thread serves draws: k = floor(u n) of the valid pixels in row-major order is found by a binary search over the
// prefix array for its word and by clearing the word's lowest (k - prefix) set bits for its bit; the pixel is back-projected in double and
// rounded once.  No atomics, no workspace, no allocation, nothing read back: capturable, and the same draws give the same bits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "hifihr_internal.h"
#include "render_math.h"

namespace hifihr {
namespace {

constexpr int kPtsThreads = 256;
constexpr int kPtsWaves = kPtsThreads / 64;
constexpr int kPtsMaxWords = kDepthPointsMaxPixels / 64;      // 4096

struct DepthPointsArgs {
  const float* depths;           // [B][H][W]
  const float* K;                // [B][3][3]
  const void* mask;              // [B][H][W] float32 or int64, or NULL
  const float* draws;            // [B][P] in [0, 1)
  const float* origin;           // [B][3] or NULL
  int mask_i64, HW, W, P;
  float* points;                 // [B][P][3]
  int* count;                    // [B]
  int* index;                    // [B][P] or NULL: the chosen pixel r W + q (-1 without a valid pixel)
};

__global__ __launch_bounds__(kPtsThreads) void depth_points_kernel(DepthPointsArgs a) {
  __shared__ unsigned long long words[kPtsMaxWords];
  __shared__ int prefix[kPtsMaxWords];
  __shared__ int part[kPtsThreads];
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int nwords = (a.HW + 63) >> 6;
  const float* dep = a.depths + (size_t)b * a.HW;
  const float* mf = (a.mask && !a.mask_i64) ? static_cast<const float*>(a.mask) + (size_t)b * a.HW : nullptr;
  const long long* ml = (a.mask && a.mask_i64) ? static_cast<const long long*>(a.mask) + (size_t)b * a.HW : nullptr;
  for (int w = wave; w < nwords; w += kPtsWaves) {             // (the bound is the same for every lane of a wave: all of them vote)
    const int p = w * 64 + lane;
    bool ok = false;
    if (p < a.HW) {
      ok = dep[p] > 0.f;
      if (mf) ok = ok && mf[p] != 0.f;
      if (ml) ok = ok && ml[p] != 0;
    }
    const unsigned long long m = __ballot(ok);
    if (lane == 0) words[w] = m;
  }
  __syncthreads();
  // exclusive prefix counts: thread t owns the words [t per, (t + 1) per), sums them, takes the sum of the shares before its own
  const int per = (nwords + kPtsThreads - 1) / kPtsThreads;
  const int w0 = t * per, w1 = (w0 + per < nwords) ? w0 + per : nwords;
  int mine = 0;
  for (int w = w0; w < w1; ++w) mine += __popcll(words[w]);
  part[t] = mine;
  __syncthreads();
  int base = 0, n = 0;
  for (int j = 0; j < kPtsThreads; ++j) {
    const int v = part[j];
    if (j < t) base += v;
    n += v;
  }
  for (int w = w0; w < w1; ++w) {
    prefix[w] = base;
    base += __popcll(words[w]);
  }
  if (t == 0) a.count[b] = n;
  __syncthreads();
  // K^-1 = adj(K) / det(K), closed form in double (no contraction: the file is compiled with -ffp-contract=off)
  const float* Kf = a.K + (size_t)b * 9;
  const double k00 = Kf[0], k01 = Kf[1], k02 = Kf[2], k10 = Kf[3], k11 = Kf[4], k12 = Kf[5], k20 = Kf[6], k21 = Kf[7], k22 = Kf[8];
  const double c00 = k11 * k22 - k12 * k21, c01 = k02 * k21 - k01 * k22, c02 = k01 * k12 - k02 * k11;
  const double c10 = k12 * k20 - k10 * k22, c11 = k00 * k22 - k02 * k20, c12 = k02 * k10 - k00 * k12;
  const double c20 = k10 * k21 - k11 * k20, c21 = k01 * k20 - k00 * k21, c22 = k00 * k11 - k01 * k10;
  const double det = (k00 * c00 + k01 * c10) + k02 * c20;
  // the pixel-centre offset of the project's camera, from the rasteriser's own sample positions: sample i of an S-wide grid sits at NDC
  // (2 i + 1) / S - 1 (pix_to_ndc), i.e. at pixel coordinate i + 0.5 under Model.camera_from_K
  const double c = 0.5 * (1.0 + (double)pix_to_ndc(0, 1));
  double ox = 0.0, oy = 0.0, oz = 0.0;
  if (a.origin) { ox = a.origin[b * 3]; oy = a.origin[b * 3 + 1]; oz = a.origin[b * 3 + 2]; }
  for (int i = t; i < a.P; i += kPtsThreads) {
    float* o = a.points + ((size_t)b * a.P + i) * 3;
    if (n == 0) {                                              // no valid pixel: the sample's points sit at the origin
      o[0] = 0.f; o[1] = 0.f; o[2] = 0.f;
      if (a.index) a.index[(size_t)b * a.P + i] = -1;
      continue;
    }
    const float f = floorf(a.draws[(size_t)b * a.P + i] * (float)n);
    const int k = f >= (float)n ? n - 1 : (f > 0.f ? (int)f : 0);     // u (float)n can round up to n; a draw outside [0, 1) (or NaN) is clamped
    int lo = 0, hi = nwords - 1;                               // the last word whose prefix is <= k
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (prefix[mid] <= k) lo = mid; else hi = mid - 1;
    }
    unsigned long long m = words[lo];
    for (int r = k - prefix[lo]; r > 0; --r) m &= m - 1;      // drop the r lowest set bits
    const int pix = lo * 64 + __ffsll(m) - 1;
    const int row = pix / a.W, col = pix - row * a.W;
    const double d = dep[pix];
    const double x = ((double)col + c) * d, y = ((double)row + c) * d;
    o[0] = (float)(((c00 * x + c01 * y) + c02 * d) / det - ox);
    o[1] = (float)(((c10 * x + c11 * y) + c12 * d) / det - oy);
    o[2] = (float)(((c20 * x + c21 * y) + c22 * d) / det - oz);
    if (a.index) a.index[(size_t)b * a.P + i] = pix;
  }
}

}  // namespace

hipError_t launch_depth_points(const float* depths, const float* K, const void* mask, int mask_i64, const float* draws, const float* origin,
                               int B, int H, int W, int P, float* points, int* count, int* index, hipStream_t st) {
  if (B <= 0 || P <= 0 || H <= 0 || W <= 0 || (long)H * W > kDepthPointsMaxPixels) return hipErrorInvalidValue;
  const DepthPointsArgs a{depths, K, mask, draws, origin, mask_i64, H * W, W, P, points, count, index};
  hipLaunchKernelGGL(depth_points_kernel, dim3(B), dim3(kPtsThreads), 0, st, a);
  return hipGetLastError();
}

}  // namespace hifihr
