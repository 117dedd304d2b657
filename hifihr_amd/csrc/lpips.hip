// LPIPS(net="alex"), version 0.1, forward only: the three launches of the metric that are not convolutions.
// Replaces `lpips.LPIPS(net="alex")` of the reference's evaluation pass (train_hrnet.py:563, called at :158); the five
// convolutions of the AlexNet trunk run on hifihr_conv2d_fwd with the bias + ReLU epilogue.
//
//   image_scale_to_nhwc4   the package's ScalingLayer, (x - shift[c]) / scale[c], fused with the NCHW -> NHWC4 repack
//                          (4th plane zero) the 11x11 stem reads: one launch, true division (rounds like the torch expression).
//   maxpool_notap          nn.MaxPool2d(3, 2) (no padding) for inference: no winning-tap bytes are written, nothing is kept
//                          for a backward.  Compares like ATen, (v > m) || isnan(v) from the first tap.
//   lpips_tap              one tap of the metric, on two channels-last maps f0, f1 [B][HW][C] and the tap's 1x1 `lin`
//                          weights w[C]:   n = f / (sqrt(sum_c f^2) + 1e-10),  d = sum_c w_c (n0_c - n1_c)^2,
//                          val[b] (+)= mean over pixels of d.   As ATen calls this is about a dozen launches per tap and two
//                          temporaries of the maps' size; here both maps are read once.
//                          DIRECT form: a group of G lanes holds one pixel's channels of both images in registers (V float4
//                          per lane and image), the two norms are group all-reduces (xor butterfly), then n0 - n1 is formed
//                          per channel.  The expanded form (sum w f0^2 / |f0|^2 - 2 sum w f0 f1 / |f0||f1| + ...) cancels on
//                          near-identical images, which is what a good reconstruction gives; identical maps give exactly 0 here.
//                          DETERMINISTIC: pixel -> (workgroup, group) is a function of (HW, C) alone, a group adds its pixels
//                          in ascending order, the workgroup folds its groups in a fixed order into partial[b][blk], and
//                          lpips_tap_finish adds a sample's partials in ascending order.  No float atomics.
//                          Bandwidth-bound (tap 1 at B = 32: 50 MB): every load is a float4, a group's loads of one pass
//                          cover G * 16 contiguous bytes.
#include <hip/hip_runtime.h>

#include <cfloat>

#include "hifihr_internal.h"

namespace hifihr {

// ------------------------------------------------------------------------------------------------
// ScalingLayer + repack: thread = one pixel
// ------------------------------------------------------------------------------------------------
struct Scale3 {
  float shift[3], scale[3];
};

__global__ __launch_bounds__(256) void image_scale_to_nhwc4_kernel(const float* __restrict__ img, float4* __restrict__ out, int B, int H, int W,
                                                                  Scale3 k) {
  const size_t HW = (size_t)H * W, n = (size_t)B * HW;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const size_t b = i / HW, p = i - b * HW;
    const float* s = img + b * 3 * HW + p;
    out[i] = make_float4((s[0] - k.shift[0]) / k.scale[0], (s[HW] - k.shift[1]) / k.scale[1], (s[2 * HW] - k.shift[2]) / k.scale[2], 0.f);
  }
}

hipError_t launch_image_scale_to_nhwc4(const float* img, float* out, int B, int H, int W, const float* shift3, const float* scale3,
                                       hipStream_t st) {
  Scale3 k;
  for (int c = 0; c < 3; ++c) { k.shift[c] = shift3[c]; k.scale[c] = scale3[c]; }
  size_t blocks = ((size_t)B * H * W + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(image_scale_to_nhwc4_kernel, dim3((unsigned)blocks), dim3(256), 0, st, img, reinterpret_cast<float4*>(out), B, H, W, k);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// MaxPool2d(3, 2, 0) without taps: thread = (output pixel, 4 channels); every window lies inside the image
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void maxpool3s2_notap_kernel(const float* __restrict__ x, int N, int H, int W, int C, int OH, int OW,
                                                              float* __restrict__ y) {
  const int C4 = C / 4;
  const size_t total = (size_t)N * OH * OW * C4;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int cg = (int)(i % C4);
    size_t rest = i / C4;
    const int ow = (int)(rest % OW); rest /= OW;
    const int oh = (int)(rest % OH);
    const int n = (int)(rest / OH);
    const float* base = x + (((size_t)n * H + oh * 2) * W + ow * 2) * C + cg * 4;      // rows oh*2 .. oh*2 + 2 < H, likewise columns
    float4 v[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int s = 0; s < 3; ++s) v[r * 3 + s] = *reinterpret_cast<const float4*>(base + ((size_t)r * W + s) * C);
    float4 m = v[0];
#pragma unroll
    for (int t = 1; t < 9; ++t) {
      if (v[t].x > m.x || v[t].x != v[t].x) m.x = v[t].x;
      if (v[t].y > m.y || v[t].y != v[t].y) m.y = v[t].y;
      if (v[t].z > m.z || v[t].z != v[t].z) m.z = v[t].z;
      if (v[t].w > m.w || v[t].w != v[t].w) m.w = v[t].w;
    }
    *reinterpret_cast<float4*>(y + i * 4) = m;
  }
}

hipError_t launch_maxpool_notap(const float* x, int N, int H, int W, int C, int k, int s, int p, float* y, hipStream_t st) {
  if (C < 4 || C % 4 != 0 || !(k == 3 && s == 2 && p == 0) || H < 3 || W < 3) return hipErrorInvalidValue;
  const int OH = (H - 3) / 2 + 1, OW = (W - 3) / 2 + 1;
  size_t blocks = ((size_t)N * OH * OW * (C / 4) + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(maxpool3s2_notap_kernel, dim3((unsigned)blocks), dim3(256), 0, st, x, N, H, W, C, OH, OW, y);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// LPIPS tap: workgroup = (pixel block, sample); group of G lanes = one pixel, V float4 per lane and image
// ------------------------------------------------------------------------------------------------
constexpr int kLpipsMaxBlocks = 64;       // partial[b][kLpipsMaxBlocks]: at most this many workgroups share a sample's pixels
constexpr int kLpipsMaxC = 512;           // (the cap of the (G, V) table below: 64 lanes x 2 float4)

template <int G>
__device__ __forceinline__ float group_allsum(float v) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <int G, int V>
__global__ __launch_bounds__(256) void lpips_tap_kernel(const float* __restrict__ f0, const float* __restrict__ f1, const float* __restrict__ w,
                                                       int HW, int C, float* __restrict__ partial) {
#pragma clang fp contract(off)             // n0 - n1 of identical inputs must be exactly zero: no fma(f0, inv0, -(f1 * inv1))
  constexpr int NG = 256 / G;              // pixels per workgroup and pass
  __shared__ float red[NG];
  const int b = blockIdx.y, gl = threadIdx.x % G, gi = threadIdx.x / G;
  const int C4 = C / 4;
  const float* p0 = f0 + (size_t)b * HW * C, *p1 = f1 + (size_t)b * HW * C;
  float4 wv[V];
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const int c4 = gl + v * G;
    wv[v] = c4 < C4 ? *reinterpret_cast<const float4*>(w + c4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  float acc = 0.f;
  // (every lane of a wave runs the same number of passes: the pixel index is clamped, a pass beyond HW contributes nothing)
  const int passes = (HW + NG * (int)gridDim.x - 1) / (NG * (int)gridDim.x);
  for (int it = 0; it < passes; ++it) {
    const int px = (it * (int)gridDim.x + (int)blockIdx.x) * NG + gi;
    const bool live = px < HW;
    const size_t o = (size_t)(live ? px : 0) * C;
    float4 a[V], c[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const int c4 = gl + v * G;
      const bool ok = c4 < C4;
      a[v] = ok ? *reinterpret_cast<const float4*>(p0 + o + c4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
      c[v] = ok ? *reinterpret_cast<const float4*>(p1 + o + c4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      s0 += (a[v].x * a[v].x + a[v].y * a[v].y) + (a[v].z * a[v].z + a[v].w * a[v].w);
      s1 += (c[v].x * c[v].x + c[v].y * c[v].y) + (c[v].z * c[v].z + c[v].w * c[v].w);
    }
    s0 = group_allsum<G>(s0);
    s1 = group_allsum<G>(s1);
    const float d0 = sqrtf(s0) + 1e-10f, d1 = sqrtf(s1) + 1e-10f;          // eps after the square root; an all-zero pixel gives 0 / 1e-10 = 0
    float d = 0.f;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const float ex = a[v].x / d0 - c[v].x / d1, ey = a[v].y / d0 - c[v].y / d1;
      const float ez = a[v].z / d0 - c[v].z / d1, ew = a[v].w / d0 - c[v].w / d1;
      d += (wv[v].x * (ex * ex) + wv[v].y * (ey * ey)) + (wv[v].z * (ez * ez) + wv[v].w * (ew * ew));
    }
    d = group_allsum<G>(d);
    acc += live ? d : 0.f;
  }
  if (gl == 0) red[gi] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int g = 0; g < NG; ++g) s += red[g];
    partial[(size_t)b * kLpipsMaxBlocks + blockIdx.x] = s;
  }
}

// val[b] = (accumulate ? val[b] : 0) + (partial[b][0] + partial[b][1] + ...) / HW     thread = sample
__global__ __launch_bounds__(64) void lpips_tap_finish_kernel(const float* __restrict__ partial, int B, int nblk, int HW, int accumulate,
                                                             float* __restrict__ val) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  float s = 0.f;
  for (int i = 0; i < nblk; ++i) s += partial[(size_t)b * kLpipsMaxBlocks + i];
  const float m = s / (float)HW;
  val[b] = accumulate ? val[b] + m : m;
}

int lpips_tap_max_channels() { return kLpipsMaxC; }
size_t lpips_tap_partial_floats(int B) { return (size_t)(B > 0 ? B : 0) * kLpipsMaxBlocks; }

template <int G, int V>
static void launch_tap(const float* f0, const float* f1, const float* w, int B, int HW, int C, float* partial, int& nblk, hipStream_t st) {
  constexpr int NG = 256 / G;
  nblk = (HW + NG - 1) / NG;
  if (nblk > kLpipsMaxBlocks) nblk = kLpipsMaxBlocks;
  hipLaunchKernelGGL((lpips_tap_kernel<G, V>), dim3(nblk, B), dim3(256), 0, st, f0, f1, w, HW, C, partial);
}

hipError_t launch_lpips_tap(const float* f0, const float* f1, const float* w, int B, int HW, int C, int accumulate, float* partial, float* val,
                            hipStream_t st) {
  if (B <= 0 || B > 65535 || HW <= 0 || C < 4 || C % 4 != 0 || C > kLpipsMaxC) return hipErrorInvalidValue;
  // (G lanes per pixel, V float4 per lane): the smallest group that holds C channels with V <= 3, so that no lane idles at the
  // AlexNet widths -- 64: 16 x 1, 192: 16 x 3, 384: 32 x 3, 256: 64 x 1
  int nblk = 0;
  if (C <= 64) launch_tap<16, 1>(f0, f1, w, B, HW, C, partial, nblk, st);
  else if (C <= 128) launch_tap<32, 1>(f0, f1, w, B, HW, C, partial, nblk, st);
  else if (C <= 192) launch_tap<16, 3>(f0, f1, w, B, HW, C, partial, nblk, st);
  else if (C <= 256) launch_tap<64, 1>(f0, f1, w, B, HW, C, partial, nblk, st);
  else if (C <= 384) launch_tap<32, 3>(f0, f1, w, B, HW, C, partial, nblk, st);
  else launch_tap<64, 2>(f0, f1, w, B, HW, C, partial, nblk, st);
  hipLaunchKernelGGL(lpips_tap_finish_kernel, dim3((B + 63) / 64), dim3(64), 0, st, partial, B, nblk, HW, accumulate, val);
  return hipGetLastError();
}

}  // namespace hifihr
