// Fused Adam over one flat fp32 parameter buffer (HBM-bound: 16 B read + 12 B written per parameter).
// Replaces torch.optim.Adam.step() as the reference configures it (reference train_hrnet.py:546-551:
// betas (0.9, 0.999), eps 1e-8, weight_decay 0 -- or 0.01 coupled L2 when optimizer == "AdamW", which in
// the reference is still optim.Adam) plus, for data parallel runs, the 1/world scaling of the all-reduced
// gradient, which is folded into the gradient read.
#include <hip/hip_runtime.h>

#include "hifihr_internal.h"

namespace hifihr {

// The gradient guard's device block (include/hifihr.h: hifihr_grad_norm): written by grad_norm_finish_kernel, read by the guarded Adam kernels.
struct GradGuard {          // 32 bytes
  double norm;              // sqrt(sum (grad_scale g_i)^2) of the last norm pass
  float coef;               // min(1, max_norm / (norm + 1e-6)); 0 when not finite
  int finite;               // 1: the sum of squares is a finite number
  int steps, clipped, skipped;
  int pad;
};

// kGuard: every workgroup reads {coef, finite} (uniform loads) -- the gradient scale becomes grad_scale * coef, formed once in f32 (coef 1.0f:
// the same bits as the unguarded instantiation), and a non-finite gradient skips the update: nothing is read or written, no weight decay.
template <bool kGuard>
__global__ __launch_bounds__(256) void adam_kernel_t(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, size_t n, float grad_scale, float beta1, float beta2,
                                                    float eps, float weight_decay, float step_size, float inv_sqrt_bc2,
                                                    const float* __restrict__ dyn, const GradGuard* __restrict__ guard) {
  // dyn (optional, device float[2] = {lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t)}): lets a captured hipGraph replay
  // the step with per-step scalars that the host refreshes outside the graph
  if (dyn) { step_size = dyn[0]; inv_sqrt_bc2 = dyn[1]; }
  if constexpr (kGuard) {
    if (!guard->finite) return;
    grad_scale = grad_scale * guard->coef;
  }
  const size_t n4 = n / 4;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  float4* p4 = reinterpret_cast<float4*>(p);
  const float4* g4 = reinterpret_cast<const float4*>(g);
  float4* m4 = reinterpret_cast<float4*>(m);
  float4* v4 = reinterpret_cast<float4*>(v);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    float4 pp = p4[i], gg = g4[i], mm = m4[i], vv = v4[i];
    float* pa = reinterpret_cast<float*>(&pp);
    float* ga = reinterpret_cast<float*>(&gg);
    float* ma = reinterpret_cast<float*>(&mm);
    float* va = reinterpret_cast<float*>(&vv);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float gr = ga[k] * grad_scale + weight_decay * pa[k];
      ma[k] = beta1 * ma[k] + (1.f - beta1) * gr;
      va[k] = beta2 * va[k] + (1.f - beta2) * gr * gr;
      const float denom = sqrtf(va[k]) * inv_sqrt_bc2 + eps;
      pa[k] = pa[k] - step_size * (ma[k] / denom);
    }
    p4[i] = pp; m4[i] = mm; v4[i] = vv;
  }
  // tail (n not a multiple of 4)
  for (size_t i = n4 * 4 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float gr = g[i] * grad_scale + weight_decay * p[i];
    const float mi = beta1 * m[i] + (1.f - beta1) * gr;
    const float vi = beta2 * v[i] + (1.f - beta2) * gr * gr;
    m[i] = mi; v[i] = vi;
    p[i] = p[i] - step_size * (mi / (sqrtf(vi) * inv_sqrt_bc2 + eps));
  }
}

// the two instantiations under the names the launches (and the emulator's launch log) use
constexpr auto adam_kernel = adam_kernel_t<false>;
constexpr auto adam_kernel_guarded = adam_kernel_t<true>;

// The same update with the step counter and the learning rate in DEVICE memory (round 5): the kernel derives the bias corrections itself
// (one thread per workgroup, double precision: the expressions launch_adam evaluates on the host) and the last workgroup to finish advances
// the counter -- every workgroup read it when it started, none starts after the last one has finished.  A captured step replays with
// nothing to refresh from the host: the per-step upload of {lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t)} (hifihr_adam_step_dyn) was a blit
// kernel of its own in front of every replay.
struct AdamState {          // 48 bytes (include/hifihr.h: hifihr_adam_step_counted)
  double lr, beta1, beta2;
  double pow1, pow2;        // beta1^step, beta2^step (running products: a double pow() per workgroup start costs microseconds)
  int step;                 // completed steps
  int done;                 // workgroups of the running launch that have finished (zero between launches)
};
// kGuard as in adam_kernel_t; a skipped step still arrives and still advances the counter and the running products (the host counts it too).
template <bool kGuard>
__global__ __launch_bounds__(256) void adam_kernel_counted_t(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                            float* __restrict__ v, size_t n, float grad_scale, float eps,
                                                            float weight_decay, AdamState* __restrict__ st,
                                                            const GradGuard* __restrict__ guard) {
  __shared__ float sc[4];
  int t = 0;
  double q1 = 0.0, q2 = 0.0;
  if (threadIdx.x == 0) {
    t = st->step + 1;
    const double b1 = st->beta1, b2 = st->beta2;
    q1 = st->pow1 * b1; q2 = st->pow2 * b2;                  // beta^t
    sc[0] = (float)(st->lr / (1.0 - q1));
    sc[1] = (float)(1.0 / sqrt(1.0 - q2));
    sc[2] = (float)b1; sc[3] = (float)b2;
  }
  __syncthreads();
  const float step_size = sc[0], inv_sqrt_bc2 = sc[1], beta1 = sc[2], beta2 = sc[3];
  bool run = true;
  if constexpr (kGuard) {
    run = guard->finite != 0;
    grad_scale = grad_scale * guard->coef;
  }
  const size_t n4 = run ? n / 4 : 0;
  const size_t n_end = run ? n : 0;                // (a skipped step: both loops are empty, the arrival below still happens)
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  float4* p4 = reinterpret_cast<float4*>(p);
  const float4* g4 = reinterpret_cast<const float4*>(g);
  float4* m4 = reinterpret_cast<float4*>(m);
  float4* v4 = reinterpret_cast<float4*>(v);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    float4 pp = p4[i], gg = g4[i], mm = m4[i], vv = v4[i];
    float* pa = reinterpret_cast<float*>(&pp);
    float* ga = reinterpret_cast<float*>(&gg);
    float* ma = reinterpret_cast<float*>(&mm);
    float* va = reinterpret_cast<float*>(&vv);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float gr = ga[k] * grad_scale + weight_decay * pa[k];
      ma[k] = beta1 * ma[k] + (1.f - beta1) * gr;
      va[k] = beta2 * va[k] + (1.f - beta2) * gr * gr;
      const float denom = sqrtf(va[k]) * inv_sqrt_bc2 + eps;
      pa[k] = pa[k] - step_size * (ma[k] / denom);
    }
    p4[i] = pp; m4[i] = mm; v4[i] = vv;
  }
  for (size_t i = n4 * 4 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_end; i += stride) {
    const float gr = g[i] * grad_scale + weight_decay * p[i];
    const float mi = beta1 * m[i] + (1.f - beta1) * gr;
    const float vi = beta2 * v[i] + (1.f - beta2) * gr * gr;
    m[i] = mi; v[i] = vi;
    p[i] = p[i] - step_size * (mi / (sqrtf(vi) * inv_sqrt_bc2 + eps));
  }
  __syncthreads();
  // No fence: a workgroup's reads of the state are consumed (data dependence) long before its arrival below, and the last arrival's stores
  // only have to be visible to the NEXT launch.  (__threadfence() here writes the L2 back once per workgroup -- with 140 MB of freshly
  // written moments in it: measured +110 us per launch.)
  if (threadIdx.x == 0) {
    if (atomicAdd(&st->done, 1) == (int)gridDim.x - 1) {       // (relaxed, device scope) the last workgroup
      st->step = t;
      st->pow1 = q1; st->pow2 = q2;
      st->done = 0;
    }
  }
}

constexpr auto adam_kernel_counted = adam_kernel_counted_t<false>;
constexpr auto adam_kernel_counted_guarded = adam_kernel_counted_t<true>;

// ------------------------------------------------------------------------------------------------
// The gradient guard's norm pass: sum of g_i^2 in double (HBM-bound: 4 B read per element), one partial per workgroup, then a one-workgroup
// finish that folds the partials and writes the guard block.  Two launches, the kernel boundary carries the partials: a last-arrival election
// would need an agent-scope release in every workgroup (the fence adam_kernel_counted avoids, above).  Every order is fixed -- a thread's
// elements in index order, lanes by shuffle tree, waves then partials in index order -- so the same input gives the same bits.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double block_sum_f64(double s, double* lds) {        // 256 threads; the total is returned to thread 0
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = s;
  __syncthreads();
  return (lds[0] + lds[1]) + (lds[2] + lds[3]);
}

__global__ __launch_bounds__(256) void grad_sqsum_kernel(const float* __restrict__ g, size_t n, double* __restrict__ partial) {
  __shared__ double lds[4];
  const size_t n4 = n / 4;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const float4* g4 = reinterpret_cast<const float4*>(g);
  double s0 = 0.0, s1 = 0.0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const float4 gg = g4[i];
    const double x = gg.x, y = gg.y, z = gg.z, w = gg.w;
    s0 += x * x; s1 += y * y;
    s0 += z * z; s1 += w * w;
  }
  for (size_t i = n4 * 4 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const double x = g[i];
    s0 += x * x;
  }
  const double s = block_sum_f64(s0 + s1, lds);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void grad_norm_finish_kernel(const double* __restrict__ partial, int nblk, float grad_scale, float max_norm,
                                                              GradGuard* __restrict__ guard) {
  __shared__ double lds[4];
  double s = 0.0;
  for (int i = threadIdx.x; i < nblk; i += 256) s += partial[i];
  s = block_sum_f64(s, lds);
  if (threadIdx.x == 0) {
    const bool finite = fabs(s) <= 1.7976931348623157e308;          // (false for NaN and for +-inf)
    const double norm = fabs((double)grad_scale) * sqrt(s);
    float coef = 0.f;
    if (finite) {
      const double c = (double)max_norm / (norm + 1e-6);              // torch.nn.utils.clip_grad_norm_; max_norm = +inf: exactly 1
      coef = c >= 1.0 ? 1.0f : (float)c;
    }
    guard->norm = norm;
    guard->coef = coef;
    guard->finite = finite ? 1 : 0;
    guard->steps += 1;
    if (finite && coef < 1.0f) guard->clipped += 1;
    if (!finite) guard->skipped += 1;
  }
}

static size_t adam_blocks(size_t n) {
  size_t blocks = (n / 4 + 255) / 256;
  if (blocks > 2048) blocks = 2048;        // grid-stride: ~8 workgroups per CU
  if (blocks < 1) blocks = 1;
  return blocks;
}

size_t grad_guard_bytes() { return sizeof(GradGuard); }
size_t grad_norm_workspace_bytes(size_t n) { return adam_blocks(n) * sizeof(double); }

hipError_t launch_grad_norm(const float* g, size_t n, float grad_scale, float max_norm, void* guard, void* ws, hipStream_t st) {
  const size_t blocks = adam_blocks(n);
  hipLaunchKernelGGL(grad_sqsum_kernel, dim3((unsigned)blocks), dim3(256), 0, st, g, n, static_cast<double*>(ws));
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(256), 0, st, static_cast<const double*>(ws), (int)blocks, grad_scale, max_norm,
                     static_cast<GradGuard*>(guard));
  return hipGetLastError();
}

// state == NULL: the host-scalar form (launch_adam's expressions); otherwise the counted form (lr, betas and step come from the state)
hipError_t launch_adam_guarded(float* p, const float* g, float* m, float* v, size_t n, float grad_scale, float lr, float beta1, float beta2,
                               float eps, float weight_decay, int step, void* state, const void* guard, hipStream_t st) {
  const size_t blocks = adam_blocks(n);
  if (state) {
    hipLaunchKernelGGL(adam_kernel_counted_guarded, dim3((unsigned)blocks), dim3(256), 0, st, p, g, m, v, n, grad_scale, eps, weight_decay,
                       static_cast<AdamState*>(state), static_cast<const GradGuard*>(guard));
    return hipGetLastError();
  }
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  const float step_size = (float)((double)lr / bc1);
  const float inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
  hipLaunchKernelGGL(adam_kernel_guarded, dim3((unsigned)blocks), dim3(256), 0, st, p, g, m, v, n, grad_scale, beta1, beta2, eps,
                     weight_decay, step_size, inv_sqrt_bc2, (const float*)nullptr, static_cast<const GradGuard*>(guard));
  return hipGetLastError();
}

size_t adam_state_bytes() { return sizeof(AdamState); }

hipError_t launch_adam_counted(float* p, const float* g, float* m, float* v, size_t n, float grad_scale, float eps, float weight_decay,
                               void* state, hipStream_t st) {
  size_t blocks = (n / 4 + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(adam_kernel_counted, dim3((unsigned)blocks), dim3(256), 0, st, p, g, m, v, n, grad_scale, eps, weight_decay,
                     static_cast<AdamState*>(state), (const GradGuard*)nullptr);
  return hipGetLastError();
}

hipError_t launch_adam(float* p, const float* g, float* m, float* v, size_t n, float grad_scale, float lr, float beta1,
                       float beta2, float eps, float weight_decay, int step, const float* dyn, hipStream_t st) {
  float step_size = 0.f, inv_sqrt_bc2 = 0.f;
  if (!dyn) {
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    step_size = (float)((double)lr / bc1);
    inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
  }
  size_t blocks = (n / 4 + 255) / 256;
  if (blocks > 2048) blocks = 2048;        // grid-stride: ~8 workgroups per CU
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(adam_kernel, dim3((unsigned)blocks), dim3(256), 0, st, p, g, m, v, n, grad_scale, beta1, beta2, eps,
                     weight_decay, step_size, inv_sqrt_bc2, dyn, (const GradGuard*)nullptr);
  return hipGetLastError();
}

}  // namespace hifihr
