// LPIPS(net="alex"), version 0.1: the three launches of the metric that are not convolutions, and (second half of the file) their backward.
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

// ================================================================================================
// The backward of the three launches above: what LPIPS(differentiable=True) and the `lpips` loss term add (gradient with respect to the
// FIRST image only; the second is the target, a constant).
//
//   lpips_tap_bwd              gf0 (+)= gval[b] / HW * d d / d f0 per pixel, ONE pass: the forward's group of G lanes holds the pixel's channels
//                              of both maps in registers again (the same (G, V) table, the same pixel -> (workgroup, group) mapping), three
//                              group all-reduces (|f0|^2, |f1|^2, t = sum_c q_c f0_c with q_c = 2 w_c (n0_c - n1_c)), then
//                                  d d / d f0_k = q_k / D0 - f0_k t / (r0 D0^2)      r0 = |f0|, D0 = r0 + 1e-10
//                              CONVENTION: on an all-zero pixel of f0 (r0 == 0) the second term is taken as 0 -- its numerator f0_k t is 0;
//                              autograd through sqrt gives NaN there -- and q_k / D0 remains.  Nothing is summed across pixels: no partials,
//                              no atomics, every output element has one writer.  fp contract(off) as in the forward: identical maps give
//                              n0 - n1 == 0 exactly, hence q == 0, t == 0 and a gradient of exactly 0.
//                              MASK (hifihr_lpips_tap_bwd_relu): f0 is a ReLU's output, as every AlexNet tap is; the sum (arriving gradient +
//                              tap gradient) is multiplied by [f0 > 0] as it is stored -- the ReLU's backward, for which the maps would
//                              otherwise be read and written once more (and hifihr_bias_relu_bwd stops at 256 channels; tap 3 has 384).
//   lpips_maxpool_fwd / _bwd   nn.MaxPool2d(3, 2) with a backward.  TAPLESS: the forward is the inference kernel above (no winning-tap bytes);
//                              the backward recomputes each window's winner from the saved INPUT, as a gather: thread = (input pixel, 4
//                              channels) looks at the at most 2 x 2 windows that cover it and adds the gy of those it wins, in ascending
//                              (oh, ow) order.  Tie rule = the forward's (v > m) || isnan(v) scan from the first tap: the first maximum in
//                              row-major window order wins (ATen).  Rows / columns that no window covers get exactly 0.  No atomics.
//   image_scale_to_nhwc4_bwd   gimg[B][3][H][W] = g4[B][H][W][c] / scale[c] (the forward's true division), the fourth plane is dropped.
// ================================================================================================
template <int G, int V, bool MASK>
__global__ __launch_bounds__(256) void lpips_tap_bwd_kernel(const float* __restrict__ f0, const float* __restrict__ f1, const float* __restrict__ w,
                                                           const float* __restrict__ gval, int HW, int C, int accumulate, float* __restrict__ gf0) {
#pragma clang fp contract(off)             // as the forward: n0 - n1 of identical inputs must be exactly zero
  constexpr int NG = 256 / G;
  const int b = blockIdx.y, gl = threadIdx.x % G, gi = threadIdx.x / G;
  const int C4 = C / 4;
  const float* p0 = f0 + (size_t)b * HW * C, *p1 = f1 + (size_t)b * HW * C;
  float* po = gf0 + (size_t)b * HW * C;
  const float gs = gval[b] / (float)HW;
  float4 wv[V];
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const int c4 = gl + v * G;
    wv[v] = c4 < C4 ? *reinterpret_cast<const float4*>(w + c4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  // (every lane of a wave runs the same number of passes and takes part in every all-reduce: the pixel index is clamped, a pass beyond HW stores nothing)
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
    const float r0 = sqrtf(s0), d0 = r0 + 1e-10f, d1 = sqrtf(s1) + 1e-10f;
    float4 q[V];
    float t = 0.f;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      q[v].x = 2.f * wv[v].x * (a[v].x / d0 - c[v].x / d1);
      q[v].y = 2.f * wv[v].y * (a[v].y / d0 - c[v].y / d1);
      q[v].z = 2.f * wv[v].z * (a[v].z / d0 - c[v].z / d1);
      q[v].w = 2.f * wv[v].w * (a[v].w / d0 - c[v].w / d1);
      t += (q[v].x * a[v].x + q[v].y * a[v].y) + (q[v].z * a[v].z + q[v].w * a[v].w);
    }
    t = group_allsum<G>(t);
    const float u = r0 > 0.f ? (t / d0) / (r0 * d0) : 0.f;      // the radial part; 0 on an all-zero pixel (the convention above)
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const int c4 = gl + v * G;
      if (live && c4 < C4) {
        float4* dst = reinterpret_cast<float4*>(po + o + c4 * 4);
        float4 g = make_float4(gs * (q[v].x / d0 - a[v].x * u), gs * (q[v].y / d0 - a[v].y * u), gs * (q[v].z / d0 - a[v].z * u),
                               gs * (q[v].w / d0 - a[v].w * u));
        if (accumulate) {
          const float4 old = *dst;
          g = make_float4(old.x + g.x, old.y + g.y, old.z + g.z, old.w + g.w);
        }
        if (MASK)                         // f0 is a ReLU's output: the gradient of its pre-activation
          g = make_float4(a[v].x > 0.f ? g.x : 0.f, a[v].y > 0.f ? g.y : 0.f, a[v].z > 0.f ? g.z : 0.f, a[v].w > 0.f ? g.w : 0.f);
        *dst = g;
      }
    }
  }
}

template <int G, int V>
static void launch_tap_bwd(const float* f0, const float* f1, const float* w, const float* gval, int B, int HW, int C, int accumulate, int relu_mask,
                           float* gf0, hipStream_t st) {
  constexpr int NG = 256 / G;
  int nblk = (HW + NG - 1) / NG;          // the forward's grid: pixel -> (workgroup, group) is a function of (HW, C) alone
  if (nblk > kLpipsMaxBlocks) nblk = kLpipsMaxBlocks;
  if (relu_mask) hipLaunchKernelGGL((lpips_tap_bwd_kernel<G, V, true>), dim3(nblk, B), dim3(256), 0, st, f0, f1, w, gval, HW, C, accumulate, gf0);
  else hipLaunchKernelGGL((lpips_tap_bwd_kernel<G, V, false>), dim3(nblk, B), dim3(256), 0, st, f0, f1, w, gval, HW, C, accumulate, gf0);
}

hipError_t launch_lpips_tap_bwd(const float* f0, const float* f1, const float* w, const float* gval, int B, int HW, int C, int accumulate,
                                int relu_mask, float* gf0, hipStream_t st) {
  if (B <= 0 || B > 65535 || HW <= 0 || C < 4 || C % 4 != 0 || C > kLpipsMaxC) return hipErrorInvalidValue;
  if (C <= 64) launch_tap_bwd<16, 1>(f0, f1, w, gval, B, HW, C, accumulate, relu_mask, gf0, st);          // the forward's (G, V) table
  else if (C <= 128) launch_tap_bwd<32, 1>(f0, f1, w, gval, B, HW, C, accumulate, relu_mask, gf0, st);
  else if (C <= 192) launch_tap_bwd<16, 3>(f0, f1, w, gval, B, HW, C, accumulate, relu_mask, gf0, st);
  else if (C <= 256) launch_tap_bwd<64, 1>(f0, f1, w, gval, B, HW, C, accumulate, relu_mask, gf0, st);
  else if (C <= 384) launch_tap_bwd<32, 3>(f0, f1, w, gval, B, HW, C, accumulate, relu_mask, gf0, st);
  else launch_tap_bwd<64, 2>(f0, f1, w, gval, B, HW, C, accumulate, relu_mask, gf0, st);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// MaxPool2d(3, 2, 0) with a backward.  forward = the tapless kernel; backward: thread = (input pixel, 4 channels)
// ------------------------------------------------------------------------------------------------
hipError_t launch_lpips_maxpool_fwd(const float* x, int N, int H, int W, int C, float* y, hipStream_t st) {
  return launch_maxpool_notap(x, N, H, W, C, 3, 2, 0, y, st);
}

__global__ __launch_bounds__(256) void lpips_maxpool_bwd_kernel(const float* __restrict__ gy, const float* __restrict__ x, int N, int H, int W, int C,
                                                               int OH, int OW, float* __restrict__ dx) {
  const int C4 = C / 4;
  const size_t total = (size_t)N * H * W * C4;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int cg = (int)(i % C4);
    size_t rest = i / C4;
    const int iw = (int)(rest % W); rest /= W;
    const int ih = (int)(rest % H);
    const int n = (int)(rest / H);
    // windows oh with 2 oh <= ih <= 2 oh + 2 that exist: an even row has two (oh = ih/2 - 1, ih/2), an odd row one, a row past the last window none
    const int oh_lo = ih >= 2 ? (ih - 1) / 2 : 0, oh_hi = min(ih / 2, OH - 1);
    const int ow_lo = iw >= 2 ? (iw - 1) / 2 : 0, ow_hi = min(iw / 2, OW - 1);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int oh = oh_lo; oh <= oh_hi; ++oh)
      for (int ow = ow_lo; ow <= ow_hi; ++ow) {
        const float* base = x + (((size_t)n * H + oh * 2) * W + ow * 2) * C + cg * 4;      // rows oh*2 .. oh*2 + 2 < H: oh <= OH - 1
        const int mine = (ih - oh * 2) * 3 + (iw - ow * 2);                                // this pixel's tap in the window, 0 .. 8
        float4 m = *reinterpret_cast<const float4*>(base);
        int wx = 0, wy = 0, wz = 0, ww = 0;
#pragma unroll
        for (int t = 1; t < 9; ++t) {
          const float4 v = *reinterpret_cast<const float4*>(base + ((size_t)(t / 3) * W + (t % 3)) * C);
          if (v.x > m.x || v.x != v.x) { m.x = v.x; wx = t; }
          if (v.y > m.y || v.y != v.y) { m.y = v.y; wy = t; }
          if (v.z > m.z || v.z != v.z) { m.z = v.z; wz = t; }
          if (v.w > m.w || v.w != v.w) { m.w = v.w; ww = t; }
        }
        const float4 g = *reinterpret_cast<const float4*>(gy + (((size_t)n * OH + oh) * OW + ow) * C + cg * 4);
        if (wx == mine) acc.x += g.x;
        if (wy == mine) acc.y += g.y;
        if (wz == mine) acc.z += g.z;
        if (ww == mine) acc.w += g.w;
      }
    *reinterpret_cast<float4*>(dx + i * 4) = acc;
  }
}

hipError_t launch_lpips_maxpool_bwd(const float* gy, const float* x, int N, int H, int W, int C, float* dx, hipStream_t st) {
  if (N <= 0 || C < 4 || C % 4 != 0 || H < 3 || W < 3) return hipErrorInvalidValue;
  const int OH = (H - 3) / 2 + 1, OW = (W - 3) / 2 + 1;
  size_t blocks = ((size_t)N * H * W * (C / 4) + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(lpips_maxpool_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, st, gy, x, N, H, W, C, OH, OW, dx);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// ScalingLayer + repack, backward: thread = one pixel
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void image_scale_to_nhwc4_bwd_kernel(const float4* __restrict__ g4, float* __restrict__ gimg, int B, int H, int W,
                                                                      Scale3 k) {
  const size_t HW = (size_t)H * W, n = (size_t)B * HW;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const size_t b = i / HW, p = i - b * HW;
    const float4 g = g4[i];
    float* d = gimg + b * 3 * HW + p;
    d[0] = g.x / k.scale[0];
    d[HW] = g.y / k.scale[1];
    d[2 * HW] = g.z / k.scale[2];
  }
}

hipError_t launch_image_scale_to_nhwc4_bwd(const float* g4, float* gimg, int B, int H, int W, const float* scale3, hipStream_t st) {
  Scale3 k;
  for (int c = 0; c < 3; ++c) { k.shift[c] = 0.f; k.scale[c] = scale3[c]; }
  size_t blocks = ((size_t)B * H * W + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(image_scale_to_nhwc4_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, st, reinterpret_cast<const float4*>(g4), gimg, B, H, W, k);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Backward-data of a STRIDED filter with more than 62 taps onto an NHWC4 image -- the 11x11 / stride 4 AlexNet stem -- which the
// implicit-GEMM gather of csrc/conv.hip does not take (its tap mask holds 62 taps; its generic gather has no strided backward-data).
// A direct gather:
//   dx[n][ih][iw][c] = sum over (r, s, k) with oh * stride - pad + r == ih, ow * stride - pad + s == iw of dy[n][oh][ow][k] w[k][r][s][c]
// workgroup = 64 input pixels of ONE phase (ih % stride, iw % stride) of one sample x 4 lanes that split K: the taps that reach a pixel depend on
// its phase alone, so the workgroup first copies ITS <= ceil(R/stride) x ceil(S/stride) taps of the filter into LDS ([tap][k] float4, read from
// the forward's own [K][R][S][4] layout: no transpose; 9 KB for the stem) and every lane then walks the same tap list.  The 4 lanes of a pixel
// read 64 contiguous bytes of dy per step (thread = pixel alone reads one cache line per lane: measured 1.1 ms at B = 32, 224^2).
// Fixed summation order per output (r, s ascending; per lane k ascending in four interleaved partial sums; then an xor tree over the 4 lanes),
// no atomics; a pixel no tap reaches gets 0.
// ------------------------------------------------------------------------------------------------
constexpr int kStemMaxTapK = 1024;       // float4 slots of LDS: taps of one phase x K (the stem: 9 x 64 = 576)

__global__ __launch_bounds__(256) void lpips_stem_bwd_data_kernel(const float* __restrict__ dy, const float* __restrict__ w, float* __restrict__ dx, int H,
                                                                 int W, int K, int R, int S, int stride, int pad, int OH, int OW) {
  __shared__ float4 w_s[kStemMaxTapK];
  const int n = blockIdx.z, ph = (int)blockIdx.y / stride, pw = (int)blockIdx.y % stride;
  const int JH = ph < H ? (H - ph + stride - 1) / stride : 0, JW = pw < W ? (W - pw + stride - 1) / stride : 0;
  const int total = JH * JW;
  const int r0 = (ph + pad) % stride, s0 = (pw + pad) % stride;      // the first tap of this phase; the others follow every `stride`
  const int nr = r0 < R ? (R - r0 + stride - 1) / stride : 0, ns = s0 < S ? (S - s0 + stride - 1) / stride : 0;
  for (int i = threadIdx.x; i < nr * ns * K; i += 256) {
    const int tap = i / K, k = i - tap * K;
    const int r = r0 + (tap / ns) * stride, q = s0 + (tap % ns) * stride;
    w_s[i] = *reinterpret_cast<const float4*>(w + (((size_t)k * R + r) * S + q) * 4);
  }
  __syncthreads();
  const int kl = threadIdx.x & 3, pl = threadIdx.x >> 2;
  // (every lane runs the same number of rounds and takes part in every shuffle: the pixel index is clamped, a round beyond `total` stores nothing)
  const int rounds = (total + 64 * (int)gridDim.x - 1) / (64 * (int)gridDim.x);
  for (int it = 0; it < rounds; ++it) {
    const int j0 = (it * (int)gridDim.x + (int)blockIdx.x) * 64 + pl;
    const bool live = j0 < total;
    const int j = live ? j0 : 0;
    const int ih = (j / JW) * stride + ph, iw = (j % JW) * stride + pw;
    float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0, a2 = a0, a3 = a0;
    for (int tr = 0; tr < nr; ++tr) {
      const int dh = ih + pad - (r0 + tr * stride);                    // a multiple of stride (negative: above the first output row)
      const int oh = dh / stride;
      if (dh < 0 || oh >= OH) continue;
      for (int ts = 0; ts < ns; ++ts) {
        const int dw = iw + pad - (s0 + ts * stride);
        const int ow = dw / stride;
        if (dw < 0 || ow >= OW) continue;
        const float* g = dy + (((size_t)n * OH + oh) * OW + ow) * K + kl * 4;
        const float4* f = w_s + (tr * ns + ts) * K + kl * 4;
        for (int k = 0; k < K; k += 16) {
          const float4 gv = *reinterpret_cast<const float4*>(g + k);
          const float4 w0 = f[k], w1 = f[k + 1], w2 = f[k + 2], w3 = f[k + 3];
          a0.x += gv.x * w0.x; a0.y += gv.x * w0.y; a0.z += gv.x * w0.z; a0.w += gv.x * w0.w;
          a1.x += gv.y * w1.x; a1.y += gv.y * w1.y; a1.z += gv.y * w1.z; a1.w += gv.y * w1.w;
          a2.x += gv.z * w2.x; a2.y += gv.z * w2.y; a2.z += gv.z * w2.z; a2.w += gv.z * w2.w;
          a3.x += gv.w * w3.x; a3.y += gv.w * w3.y; a3.z += gv.w * w3.z; a3.w += gv.w * w3.w;
        }
      }
    }
    float4 t = make_float4((a0.x + a1.x) + (a2.x + a3.x), (a0.y + a1.y) + (a2.y + a3.y), (a0.z + a1.z) + (a2.z + a3.z), (a0.w + a1.w) + (a2.w + a3.w));
#pragma unroll
    for (int o = 1; o <= 2; o <<= 1) {
      t.x += __shfl_xor(t.x, o, 64); t.y += __shfl_xor(t.y, o, 64); t.z += __shfl_xor(t.z, o, 64); t.w += __shfl_xor(t.w, o, 64);
    }
    if (live && kl == 0) *reinterpret_cast<float4*>(dx + (((size_t)n * H + ih) * W + iw) * 4) = t;
  }
}

bool lpips_stem_bwd_data_supported(int N, int H, int W, int C, int K, int R, int S, int stride, int pad) {
  if (!(N > 0 && N <= 65535 && H > 0 && W > 0 && C == 4 && K >= 16 && K % 16 == 0 && R > 0 && S > 0 && stride > 1 && stride <= 16 && pad >= 0 &&
        H + 2 * pad >= R && W + 2 * pad >= S && R * S > 62 && (long)H * W < (1L << 30)))
    return false;
  return (long)((R + stride - 1) / stride) * ((S + stride - 1) / stride) * K <= kStemMaxTapK;
}

hipError_t launch_lpips_stem_bwd_data(const float* dy, const float* w, float* dx, int N, int H, int W, int C, int K, int R, int S, int stride, int pad,
                                      hipStream_t st) {
  if (!lpips_stem_bwd_data_supported(N, H, W, C, K, R, S, stride, pad)) return hipErrorInvalidValue;
  const int OH = (H + 2 * pad - R) / stride + 1, OW = (W + 2 * pad - S) / stride + 1;
  const int JH = (H + stride - 1) / stride, JW = (W + stride - 1) / stride;       // the largest phase
  long blocks = ((long)JH * JW + 63) / 64;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(lpips_stem_bwd_data_kernel, dim3((unsigned)blocks, (unsigned)(stride * stride), (unsigned)N), dim3(256), 0, st, dy, w, dx, H, W, K, R,
                     S, stride, pad, OH, OW);
  return hipGetLastError();
}

}  // namespace hifihr
