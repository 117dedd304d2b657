// Test-time fit of the MANO parameters to 2-D / 3-D keypoints for gfx950: the whole optimisation in ONE launch.
//
// Replaces the reference's mano_fitting (utils/traineval_util.py:505-595: 151 Adam iterations, each a ManoLayer forward, a projection,
// the loss terms, autograd and an optimiser step -- a few thousand small launches per batch) with
//   mano_fit_kernel   grid B x 1024 threads, one workgroup per hand.  The hand's 61 parameters, Adam moments, 778 vertices and their
//                     gradients live in LDS (about 50 KB, static); every iteration runs inside the kernel with __syncthreads() as its
//                     only synchronisation.  The 1.4 MB of tables are read from L2 twice per iteration (blend forward, blend transpose);
//                     nothing but one trace row of 8 floats goes to HBM between iterations.  No atomics, no cross-workgroup traffic.
// include/hifihr.h (hifihr_mano_fit) states the objective, the operation order and the decided corners.
//
// The MANO phases restate those of mano_lbs.hip (prologue, blend + skin, joint regression, and the backward phases 2a .. 5 of
// mano_bwd_kernel) on top of the shared scalar routines of mano_math.h; mano_lbs.hip itself is untouched, so its kernels compile as before.
#include <hip/hip_runtime.h>

#include "hifihr_internal.h"
#include "mano_math.h"

namespace hifihr {
namespace {

constexpr int kFitThreads = 1024;   // 16 waves: a wave per regressed joint, a thread per vertex; 4 waves per SIMD = at most 128 VGPRs per lane
constexpr int kFitWaves = kFitThreads / 64;
constexpr int kFitPar = 61;         // pose[48] | beta[10] | root[3]
constexpr float kFitMinZ = 1e-4f;   // a joint at or below this depth takes no part in the two 2-D terms (include/hifihr.h)
constexpr int kBlendGroup = 9;      // pose blend-shape rows in flight per lane (27 loads)

// xyz_from_vertice: FreiHAND slot -> regressed MANO joint id (>= 0) or -(vertex id) - 1 for the five tips (as in mano_lbs.hip)
__device__ __constant__ int c_fit_xyz_src[21] = {0, 13, 14, 15, -744 - 1, 1, 2, 3, -320 - 1, 4, 5, 6, -443 - 1,
                                                 10, 11, 12, -555 - 1, 7, 8, 9, -672 - 1};

// bone `k` of the 20: child k + 1, parent 0 for the first bone of a finger, k otherwise (losses.hip: kBoneParent / kBoneChild)
__device__ __forceinline__ int fit_bone_parent(int bone) { return (bone % 4 == 0) ? 0 : bone; }

struct FitLds {
  // ---- the MANO state of mano_lbs.hip's ManoSmall ----
  float pose[48];
  float beta[kNB];
  float fp[48];             // full axis-angle pose
  float Rl[kNJ * 9];
  float Rg[kNJ * 9];
  float tg[kNJ * 3];
  float J[kNJ * 3];
  float Ap[kNJ * 12];
  float pm[kNP];            // pose_map = R - I for joints 1..15
  // ---- the fit ----
  float root[3];
  float m[kFitPar], v[kFitPar], g[kFitPar], cand[kFitPar], m_new[kFitPar], v_new[kFitPar];
  float K[9], kp[42], con[21], kp3[63], con3[21], plo[48], phi[48], pw[48];
  float j16[kNJ * 3], j21[63], jrel[63];
  float uv[42], dxy[42], dist[21], w2[21], ceff[21];       // per joint: projection, residual, |residual|, c^2 (0 when left out), c (0 when left out)
  float p2[21];                                            // (K X)_z
  float s_rho[21], s_e3[21], s_pix[21], s_pixn[21];        // per-joint addends of the sums
  float bone_t[20], bone_g[40];                            // per bone: its term (confidence included) and d term / d (child - parent)
  float prior_e[48], prior_s[48];                          // per element of fp: its addend and the sign of its slope (times w)
  float terms[8];                                          // the trace row
  float coef2d, coef3d;                                    // w2d / sum c^2 and w3d / sum c3 (0 when the sum is 0)
  int bad;
  float gX[63], gj21[63], gj16[kNJ * 3], gr[3];
  alignas(16) float sv[3 * kNVP];      // skinned vertices, SoA
  alignas(16) float vp[3 * kNVP];      // v_posed, SoA
  alignas(16) float gv[3 * kNVP];      // gradient wrt the skinned vertices, SoA
  alignas(16) float gvp[3 * kNVP];     // gradient wrt v_posed, SoA (same indexing as a table row)
  float gAp[kNJ * 12];
  float gRg[kNJ * 9];
  float gtg[kNJ * 3];
  float gJ[kNJ * 3];
  float gRl[kNJ * 9];
  float gpm[kNP];
  float gbeta_blend[kNB];
  float gfp[48];
  float root_acc[5 * 15];   // per finger: gRg0[9], gtg0[3], gJ0[3]
};
static_assert(sizeof(FitLds) <= 64 * 1024, "static LDS");

struct FitArgs {
  float* pose; float* beta; float* root;
  const float* K; const float* kp2d; const float* conf2d; const float* kp3d; const float* conf3d;
  const float* plo; const float* phi; const float* pw; const float* lr;
  int iters, root_id;
  float w[6];               // w2d, wbone, w3d, wprior, wshape, wpca
  float mult[4];            // root rotation, pose coefficients, shape, root position
  float* trace; float* grad0; int32_t* done;
};

__device__ __forceinline__ float fit_wave_sum(float x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
  return x;
}

// The thread index as a value the compiler cannot prove loop-invariant: the addresses formed from it are then recomputed in each phase of each
// iteration (a few VALU instructions) instead of being hoisted out of the iteration loop, where they overflowed the 128 VGPRs into scratch.
// Read with hipcc of ROCm 7.2 (AMD clang 22.0.0git, roc-7.2.0), -O3, gfx950: 350 spilled VGPRs / 1300 B of scratch per lane without this, 39 / 120 B with it
// (-Rpass-analysis=kernel-resource-usage, or tools/kernel_regs.py); when a compiler gives no spills without it, it can go.
__device__ __forceinline__ int fit_tid() {
  int tid = threadIdx.x;
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(tid));
#endif
  return tid;
}

__device__ __forceinline__ bool fit_finite(float x) { return fabsf(x) <= 3.402823466e38f; }   // false for NaN and +-inf

// ---- forward: from (pose, beta, root) in LDS to the trace row L.terms; ends with a barrier ----
__device__ __forceinline__ void fit_forward(const ManoDev& t, const FitArgs& a, FitLds& L) {
  const int tid = fit_tid(), lane = tid & 63, wave = tid >> 6;
  // prologue (mano_lbs.hip: mano_prologue)
  if (tid < kNPCA) {
    float acc = 0.f;
    for (int k = 0; k < kNPCA; ++k) acc += L.pose[3 + k] * t.comps[k * kNPCA + tid];
    L.fp[3 + tid] = t.mean[tid] + acc;
  } else if (tid < 48) {
    L.fp[tid - kNPCA] = L.pose[tid - kNPCA];
  }
  if (tid >= 64 && tid < 64 + 48) {
    const int e = tid - 64;
    float acc = t.jt[e];
    for (int k = 0; k < kNB; ++k) acc += t.jsd[e * kNB + k] * L.beta[k];
    L.J[e] = acc;
  }
  if (tid == 128) L.bad = 0;
  __syncthreads();
  if (tid < kNJ) {
    rodrigues_fwd(L.fp + 3 * tid, L.Rl + 9 * tid, nullptr);
    if (tid >= 1) {
      for (int k = 0; k < 9; ++k) L.pm[(tid - 1) * 9 + k] = L.Rl[9 * tid + k] - ((k % 4 == 0) ? 1.f : 0.f);
    }
  }
  if (tid >= 64 && tid < 64 + 48) {          // the pose prior on the full axis-angle pose: strict comparisons, slope 0 at a bound
    const int i = tid - 64;
    float e = 0.f, s = 0.f;
    if (a.plo) {
      const float f = L.fp[i], w = L.pw[i];
      if (f > L.phi[i]) { e = w * (f - L.phi[i]); s = w; }
      else if (f < L.plo[i]) { e = w * (L.plo[i] - f); s = -w; }
      else if (!(f == f)) { e = f; }                                  // a NaN pose is reported, not hidden by the comparisons
    }
    L.prior_e[i] = e; L.prior_s[i] = s;
  }
  __syncthreads();
  if (tid == 0) chain_fwd_root(L.Rl, L.J, L.Rg, L.tg);
  __syncthreads();
  if (tid < 5) chain_fwd_finger(tid, L.Rl, L.J, L.Rg, L.tg);
  __syncthreads();
  if (tid < kNJ) chain_make_ap(tid, L.J, L.Rg, L.tg, L.Ap);
  __syncthreads();

  // blend shapes and skinning, a vertex per thread (mano_fwd_kernel without the centring: the root-relative step below removes any offset)
  static_assert(kFitThreads >= kNVP, "a vertex per thread");
  if (tid < kNVP) {
    const int v = tid;
    float vp[3] = {0.f, 0.f, 0.f}, o[3] = {0.f, 0.f, 0.f};
    if (v < kNV) {
#pragma unroll
      for (int c = 0; c < 3; ++c) vp[c] = t.tmpl[c * kNVP + v];
      for (int k = 0; k < kNB; ++k) {
        const float bk = L.beta[k];
        const float* row = t.sd + (size_t)k * 3 * kNVP + v;
        vp[0] += row[0] * bk; vp[1] += row[kNVP] * bk; vp[2] += row[2 * kNVP] * bk;
      }
      static_assert(kNP % kBlendGroup == 0, "pose blend shapes in whole groups");
#pragma unroll 1
      for (int p0 = 0; p0 < kNP; p0 += kBlendGroup) {
        float r[kBlendGroup][3];
#pragma unroll
        for (int u = 0; u < kBlendGroup; ++u) {
          const float* row = t.pd + (size_t)(p0 + u) * 3 * kNVP + v;
          r[u][0] = row[0]; r[u][1] = row[kNVP]; r[u][2] = row[2 * kNVP];
        }
#pragma unroll
        for (int u = 0; u < kBlendGroup; ++u) {
          const float pk = L.pm[p0 + u];
          vp[0] += r[u][0] * pk; vp[1] += r[u][1] * pk; vp[2] += r[u][2] * pk;
        }
      }
      float wv[kNJ];
#pragma unroll
      for (int i = 0; i < kNJ; ++i) wv[i] = t.w[i * kNVP + v];
      float T[12];
#pragma unroll
      for (int k = 0; k < 12; ++k) T[k] = 0.f;
#pragma unroll
      for (int i = 0; i < kNJ; ++i) {
#pragma unroll
        for (int k = 0; k < 12; ++k) T[k] += wv[i] * L.Ap[12 * i + k];
      }
#pragma unroll
      for (int r = 0; r < 3; ++r) o[r] = T[4 * r] * vp[0] + T[4 * r + 1] * vp[1] + T[4 * r + 2] * vp[2] + T[4 * r + 3];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) { L.vp[c * kNVP + v] = vp[c]; L.sv[c * kNVP + v] = o[c]; }
  }
  __syncthreads();
  // joint regression, a wave per regressed joint (mano_joints_fwd_kernel)
  static_assert(kFitWaves >= kNJ, "a wave per joint");
  if (wave < kNJ) {
    constexpr int kIt = (kNV + 63) / 64;
    const float* jr = t.jreg + wave * kNVP;
    float rv[kIt];
#pragma unroll
    for (int i = 0; i < kIt; ++i) { const int v = lane + 64 * i; rv[i] = v < kNV ? jr[v] : 0.f; }
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll
    for (int i = 0; i < kIt; ++i) {
      const int v = lane + 64 * i;
      if (v < kNV) { a0 += rv[i] * L.sv[v]; a1 += rv[i] * L.sv[kNVP + v]; a2 += rv[i] * L.sv[2 * kNVP + v]; }
    }
    a0 = fit_wave_sum(a0); a1 = fit_wave_sum(a1); a2 = fit_wave_sum(a2);
    if (lane == 0) { L.j16[wave * 3] = a0; L.j16[wave * 3 + 1] = a1; L.j16[wave * 3 + 2] = a2; }
  }
  __syncthreads();
  if (tid < 63) {
    const int sl = tid / 3, c = tid % 3;
    const int src = c_fit_xyz_src[sl];
    L.j21[tid] = (src >= 0) ? L.j16[src * 3 + c] : L.sv[c * kNVP + (-src - 1)];
  }
  __syncthreads();
  // per joint: root-relative step, camera space, projection, the addends of e2d / e3d / the pixel error
  if (tid < 21) {
    const int j = tid;
    float jr[3], X[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      jr[c] = L.j21[3 * j + c] - L.j21[3 * a.root_id + c];
      X[c] = jr[c] + L.root[c];
      L.jrel[3 * j + c] = jr[c];
    }
    const float* K = L.K;
    const float p0 = K[0] * X[0] + K[1] * X[1] + K[2] * X[2];
    const float p1 = K[3] * X[0] + K[4] * X[1] + K[5] * X[2];
    const float p2 = K[6] * X[0] + K[7] * X[1] + K[8] * X[2];
    const float c = L.con[j];
    const bool in = X[2] > kFitMinZ;                  // (a NaN depth compares false: E is made non-finite below)
    float u = 0.f, vv = 0.f, dx = 0.f, dy = 0.f, d = 0.f, rho = 0.f;
    if (in) {
      u = p0 / p2; vv = p1 / p2;
      dx = u - L.kp[2 * j]; dy = vv - L.kp[2 * j + 1];
      const float d2 = dx * dx + dy * dy;
      d = sqrtf(d2);
      rho = d < 5.f ? d2 / 10.f : d - 2.5f;
    }
    const float w2 = in ? c * c : 0.f;
    L.uv[2 * j] = u; L.uv[2 * j + 1] = vv; L.dxy[2 * j] = dx; L.dxy[2 * j + 1] = dy; L.dist[j] = d; L.p2[j] = p2;
    L.w2[j] = w2; L.ceff[j] = in ? c : 0.f;
    L.s_rho[j] = (X[2] == X[2]) ? rho * w2 : X[2];
    const bool seen = in && c > 0.f;
    L.s_pix[j] = seen ? d : 0.f; L.s_pixn[j] = seen ? 1.f : 0.f;
    float e3 = 0.f;
    if (a.kp3d) {
      const float ex = jr[0] - L.kp3[3 * j], ey = jr[1] - L.kp3[3 * j + 1], ez = jr[2] - L.kp3[3 * j + 2];
      e3 = L.con3[j] * (ex * ex + ey * ey + ez * ez);
    }
    L.s_e3[j] = e3;
  }
  __syncthreads();
  // per bone: |vn - von|^2 c_parent c_child and its slope wrt (child - parent)  (losses.hip: bone_term, open2d_terms_bwd_kernel)
  if (tid < 20) {
    const int bone = tid, p = fit_bone_parent(bone), ch = bone + 1;
    const float conf = L.ceff[p] * L.ceff[ch];
    float term = 0.f, gx = 0.f, gy = 0.f;
    if (conf != 0.f) {
      const float vx = L.uv[2 * ch] - L.uv[2 * p], vy = L.uv[2 * ch + 1] - L.uv[2 * p + 1];
      const float ox = L.kp[2 * ch] - L.kp[2 * p], oy = L.kp[2 * ch + 1] - L.kp[2 * p + 1];
      const float n = sqrtf(vx * vx + vy * vy), il = 1.0f / (n + 1e-4f), ig = 1.0f / (sqrtf(ox * ox + oy * oy) + 1e-4f);
      const float vnx = vx * il, vny = vy * il;
      const float dnx = vnx - ox * ig, dny = vny - oy * ig;
      term = (dnx * dnx + dny * dny) * conf;
      const float dot = dnx * vnx + dny * vny, k = 2.f * conf * il;
      gx = k * (dnx - (n > 0.f ? dot * vx / n : 0.f));
      gy = k * (dny - (n > 0.f ? dot * vy / n : 0.f));
    }
    L.bone_t[bone] = term; L.bone_g[2 * bone] = gx; L.bone_g[2 * bone + 1] = gy;
  }
  __syncthreads();
  if (wave == 0) {                                    // every sum as one wave reduction: a fixed order
    const float sw = fit_wave_sum(lane < 21 ? L.w2[lane] : 0.f), srho = fit_wave_sum(lane < 21 ? L.s_rho[lane] : 0.f);
    const float s3 = fit_wave_sum(lane < 21 ? L.s_e3[lane] : 0.f), s3w = fit_wave_sum(lane < 21 && a.kp3d ? L.con3[lane] : 0.f);
    const float spix = fit_wave_sum(lane < 21 ? L.s_pix[lane] : 0.f), spixn = fit_wave_sum(lane < 21 ? L.s_pixn[lane] : 0.f);
    const float sb = fit_wave_sum(lane < 20 ? L.bone_t[lane] : 0.f), sp = fit_wave_sum(lane < 48 ? L.prior_e[lane] : 0.f);
    const float ss = fit_wave_sum(lane < kNB ? L.beta[lane] * L.beta[lane] : 0.f);
    const float sc = fit_wave_sum(lane < kNPCA ? L.pose[3 + lane] * L.pose[3 + lane] : 0.f);
    if (lane == 0) {
    const float e2d = sw > 0.f ? srho / sw : (srho == srho ? 0.f : srho);
    const float ebone = sb / 20.f;
    const float e3d = s3w > 0.f ? s3 / s3w : (s3 == s3 ? 0.f : s3);
    const float eprior = sp / 48.f, eshape = ss / (float)kNB, epca = sc / 45.f;
    L.terms[0] = a.w[0] * e2d + a.w[1] * ebone + a.w[2] * e3d + a.w[3] * eprior + a.w[4] * eshape + a.w[5] * epca;
    L.terms[1] = e2d; L.terms[2] = ebone; L.terms[3] = e3d; L.terms[4] = eprior; L.terms[5] = eshape; L.terms[6] = epca;
    L.terms[7] = spixn > 0.f ? spix / spixn : 0.f;
    L.coef2d = sw > 0.f ? a.w[0] / sw : 0.f;
    L.coef3d = s3w > 0.f ? a.w[2] / s3w : 0.f;
    }
  }
  __syncthreads();
}

// ---- backward: from the forward's LDS state to L.g[61] = dE / d(pose, beta, root); ends with a barrier ----
__device__ __forceinline__ void fit_backward(const ManoDev& t, const FitArgs& a, FitLds& L) {
  const int tid = fit_tid(), lane = tid & 63, wave = tid >> 6;
  // through the projection and the root-relative step
  if (tid < 21) {
    const int j = tid;
    float gu = 0.f, gvv = 0.f;
    if (L.w2[j] != 0.f) {
      const float d = L.dist[j];
      const float k = L.coef2d * L.w2[j] * (d < 5.f ? 0.2f : 1.f / d);   // d rho / d uv = (uv - kp) / 5 below 5 px: exactly 0 at d = 0
      gu = k * L.dxy[2 * j]; gvv = k * L.dxy[2 * j + 1];
    }
    const float cb = a.w[1] / 20.f;
    if (j >= 1) { gu += cb * L.bone_g[2 * (j - 1)]; gvv += cb * L.bone_g[2 * (j - 1) + 1]; }        // the bone whose child j is
    if (j == 0) {
      for (int f = 0; f < 20; f += 4) { gu -= cb * L.bone_g[2 * f]; gvv -= cb * L.bone_g[2 * f + 1]; }
    } else if (j % 4 != 0) {
      gu -= cb * L.bone_g[2 * j]; gvv -= cb * L.bone_g[2 * j + 1];                                 // the bone whose parent j is
    }
    float gX[3] = {0.f, 0.f, 0.f};
    if (L.ceff[j] != 0.f || L.w2[j] != 0.f) {
      const float ip = 1.f / L.p2[j];
      const float g0 = gu * ip, g1 = gvv * ip, g2 = -(gu * L.uv[2 * j] + gvv * L.uv[2 * j + 1]) * ip;
      const float* K = L.K;
#pragma unroll
      for (int c = 0; c < 3; ++c) gX[c] = K[c] * g0 + K[3 + c] * g1 + K[6 + c] * g2;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float g = gX[c];
      if (a.kp3d) g += L.coef3d * L.con3[j] * 2.f * (L.jrel[3 * j + c] - L.kp3[3 * j + c]);
      L.gX[3 * j + c] = gX[c];
      L.gj21[3 * j + c] = g;
    }
  }
  __syncthreads();
  if (tid < 3) {                                      // root position: every joint's camera-space gradient; root joint: minus every relative one
    float gp = 0.f, gr = 0.f;
    for (int j = 0; j < 21; ++j) { gp += L.gX[3 * j + tid]; gr -= L.gj21[3 * j + tid]; }
    L.g[58 + tid] = gp;
    L.gr[tid] = gr;
  }
  __syncthreads();
  if (tid < 3) L.gj21[a.root_id * 3 + tid] += L.gr[tid];
  __syncthreads();
  if (tid < kNJ * 3) {
    const int j = tid / 3, c = tid % 3;
    float acc = 0.f;
    for (int sl = 0; sl < 21; ++sl)
      if (c_fit_xyz_src[sl] == j) acc += L.gj21[sl * 3 + c];
    L.gj16[tid] = acc;
  }
  __syncthreads();
  // through the joint regression and the tips, a vertex per thread (mano_bwd_kernel phase 0)
  if (tid < kNVP) {
    const int v = tid;
    float g0[3] = {0.f, 0.f, 0.f};
    if (v < kNV) {
      float wj[kNJ];
#pragma unroll
      for (int j = 0; j < kNJ; ++j) wj[j] = t.jreg[j * kNVP + v];
#pragma unroll
      for (int j = 0; j < kNJ; ++j) { g0[0] += wj[j] * L.gj16[j * 3]; g0[1] += wj[j] * L.gj16[j * 3 + 1]; g0[2] += wj[j] * L.gj16[j * 3 + 2]; }
      for (int sl = 4; sl < 21; sl += 4)
        if (-c_fit_xyz_src[sl] - 1 == v) { g0[0] += L.gj21[sl * 3]; g0[1] += L.gj21[sl * 3 + 1]; g0[2] += L.gj21[sl * 3 + 2]; }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) L.gv[c * kNVP + v] = g0[c];
  }
  __syncthreads();
  // phase 2a: gAp[i][4r+c] = sum_v w[v,i] gv[r][v] [vp;1][c][v], a wave per joint
  if (wave < kNJ) {
    constexpr int kIt = (kNV + 63) / 64;
    const float* wrow = t.w + wave * kNVP;
    float wv[kIt];
#pragma unroll
    for (int i = 0; i < kIt; ++i) { const int v = lane + 64 * i; wv[i] = v < kNV ? wrow[v] : 0.f; }
    float acc[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) acc[k] = 0.f;
#pragma unroll
    for (int i = 0; i < kIt; ++i) {
      const int v = lane + 64 * i;
      if (v < kNV) {
        const float w = wv[i];
        const float p[4] = {L.vp[v], L.vp[kNVP + v], L.vp[2 * kNVP + v], 1.f};
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          const float wg = w * L.gv[r * kNVP + v];
#pragma unroll
          for (int c = 0; c < 4; ++c) acc[4 * r + c] += wg * p[c];
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) {
      const float r = fit_wave_sum(acc[k]);
      if (lane == 0) L.gAp[wave * 12 + k] = r;
    }
  }
  // phase 2b: gvp[v] = sum_i w[v,i] Rg_i^T gv[v], a vertex per thread
  if (tid < kNVP) {
    const int v = tid;
    float o[3] = {0.f, 0.f, 0.f};
    if (v < kNV) {
      const float g[3] = {L.gv[v], L.gv[kNVP + v], L.gv[2 * kNVP + v]};
      float wv[kNJ];
#pragma unroll
      for (int i = 0; i < kNJ; ++i) wv[i] = t.w[i * kNVP + v];
#pragma unroll
      for (int i = 0; i < kNJ; ++i) {
        const float w = wv[i];
        const float* R = L.Rg + 9 * i;
        o[0] += w * (R[0] * g[0] + R[3] * g[1] + R[6] * g[2]);
        o[1] += w * (R[1] * g[0] + R[4] * g[1] + R[7] * g[2]);
        o[2] += w * (R[2] * g[0] + R[5] * g[1] + R[8] * g[2]);
      }
    }
    L.gvp[v] = o[0]; L.gvp[kNVP + v] = o[1]; L.gvp[2 * kNVP + v] = o[2];
  }
  __syncthreads();
  // phase 3: blend-shape transposes, a wave walks its rows two at a time (20 float4 per lane in flight)
  {
    constexpr int kRow4 = 3 * kNVP / 4;
    const float4* g4 = reinterpret_cast<const float4*>(L.gvp);
    constexpr int kIt = (kRow4 + 63) / 64;
#pragma unroll 1
    for (int row0 = wave; row0 < kNP + kNB; row0 += 2 * kFitWaves) {
      const int row1 = row0 + kFitWaves;
      const bool two = row1 < kNP + kNB;
      const float* base0 = (row0 < kNP) ? t.pd + (size_t)row0 * 3 * kNVP : t.sd + (size_t)(row0 - kNP) * 3 * kNVP;
      const float* base1 = !two ? base0 : ((row1 < kNP) ? t.pd + (size_t)row1 * 3 * kNVP : t.sd + (size_t)(row1 - kNP) * 3 * kNVP);
      const float4* r40 = reinterpret_cast<const float4*>(base0);
      const float4* r41 = reinterpret_cast<const float4*>(base1);
      float4 a0[kIt], a1[kIt];
#pragma unroll
      for (int i = 0; i < kIt; ++i) {
        const int e = lane + 64 * i;
        a0[i] = r40[e < kRow4 ? e : kRow4 - 1];
        a1[i] = r41[e < kRow4 ? e : kRow4 - 1];
      }
      float acc0 = 0.f, acc1 = 0.f;
#pragma unroll
      for (int i = 0; i < kIt; ++i) {
        const int e = lane + 64 * i;
        if (e < kRow4) {
          const float4 g = g4[e];
          acc0 += a0[i].x * g.x + a0[i].y * g.y + a0[i].z * g.z + a0[i].w * g.w;
          acc1 += a1[i].x * g.x + a1[i].y * g.y + a1[i].z * g.z + a1[i].w * g.w;
        }
      }
      acc0 = fit_wave_sum(acc0);
      acc1 = fit_wave_sum(acc1);
      if (lane == 0) {
        if (row0 < kNP) L.gpm[row0] = acc0; else L.gbeta_blend[row0 - kNP] = acc0;
        if (two) { if (row1 < kNP) L.gpm[row1] = acc1; else L.gbeta_blend[row1 - kNP] = acc1; }
      }
    }
  }
  // phase 4: fold gAp into the chain, walk the chain backwards
  if (tid < kNJ * 9) L.gRg[tid] = 0.f;
  if (tid < kNJ * 3) { L.gtg[tid] = 0.f; L.gJ[tid] = 0.f; }
  if (tid < 5 * 15) L.root_acc[tid] = 0.f;
  __syncthreads();
  if (tid < kNJ) chain_make_ap_bwd(tid, L.J, L.Rg, L.gAp, L.gRg, L.gtg, L.gJ);
  __syncthreads();
  if (tid < 5) {
    float* acc = L.root_acc + 15 * tid;
    chain_bwd_finger(tid, L.Rl, L.J, L.Rg, L.gRg, L.gtg, L.gRl, L.gJ, acc, acc + 9, acc + 12);
  }
  __syncthreads();
  if (tid < 15) {               // root: Rg_0 = Rl_0, tg_0 = J_0
    float acc = 0.f;
    for (int f = 0; f < 5; ++f) acc += L.root_acc[15 * f + tid];
    if (tid < 9) L.gRl[tid] = L.gRg[tid] + acc;
    else if (tid < 12) L.root_acc[tid] = L.gtg[tid - 9] + acc;      // reuse slot: total g(tg_0)
    else L.root_acc[tid] = L.gJ[tid - 12] + acc;                    // gJ_0 (chain part)
  }
  __syncthreads();
  if (tid < 3) L.gJ[tid] = L.root_acc[12 + tid] + L.root_acc[9 + tid];
  if (tid >= 64 && tid < 64 + kNP) L.gRl[9 + (tid - 64)] += L.gpm[tid - 64];
  __syncthreads();
  if (tid < kNJ) rodrigues_bwd(L.fp + 3 * tid, L.gRl + 9 * tid, L.gfp + 3 * tid);
  __syncthreads();
  if (tid < 48) L.gfp[tid] += (a.w[3] / 48.f) * L.prior_s[tid];     // the prior acts on the full pose
  __syncthreads();
  // phase 5: PCA transpose, shape gradient, the two quadratic priors
  if (tid < 3) {
    L.g[tid] = L.gfp[tid];
  } else if (tid < 48) {
    const int k = tid - 3;
    float acc = 0.f;
    for (int j = 0; j < kNPCA; ++j) acc += t.comps[k * kNPCA + j] * L.gfp[3 + j];
    L.g[tid] = acc + a.w[5] * (2.f / 45.f) * L.pose[tid];
  } else if (tid >= 64 && tid < 64 + kNB) {
    const int k = tid - 64;
    float acc = L.gbeta_blend[k];
    for (int e = 0; e < kNJ * 3; ++e) acc += t.jsd[e * kNB + k] * L.gJ[e];
    L.g[48 + k] = acc + a.w[4] * (2.f / (float)kNB) * L.beta[k];
  }
  __syncthreads();
}

__global__ __launch_bounds__(kFitThreads) void mano_fit_kernel(ManoDev t, FitArgs a) {
  __shared__ FitLds L;
  const int b = blockIdx.x, tid = threadIdx.x;
  if (tid < 48) L.pose[tid] = a.pose[b * 48 + tid];
  if (tid >= 64 && tid < 64 + kNB) L.beta[tid - 64] = a.beta[b * kNB + tid - 64];
  if (tid >= 96 && tid < 99) L.root[tid - 96] = a.root[b * 3 + tid - 96];
  if (tid >= 128 && tid < 128 + kFitPar) { L.m[tid - 128] = 0.f; L.v[tid - 128] = 0.f; }
  if (tid >= 192 && tid < 192 + 9) L.K[tid - 192] = a.K[b * 9 + tid - 192];
  if (tid >= 256 && tid < 256 + 42) L.kp[tid - 256] = a.kp2d[b * 42 + tid - 256];
  if (tid >= 320 && tid < 320 + 21) L.con[tid - 320] = a.conf2d[b * 21 + tid - 320];
  if (tid >= 384 && tid < 384 + 63) L.kp3[tid - 384] = a.kp3d ? a.kp3d[b * 63 + tid - 384] : 0.f;
  if (tid >= 448 && tid < 448 + 21) L.con3[tid - 448] = a.conf3d ? a.conf3d[b * 21 + tid - 448] : 0.f;
  if (tid >= 512 && tid < 512 + 48) {
    const int i = tid - 512;
    L.plo[i] = a.plo ? a.plo[i] : 0.f; L.phi[i] = a.plo ? a.phi[i] : 0.f; L.pw[i] = a.plo ? a.pw[i] : 0.f;
  }
  __syncthreads();

  double b1t = 1.0, b2t = 1.0;           // beta^t as running products in double: 1 - 0.999^t is formed without float32 cancellation
  int done = a.iters;
  float* trace = a.trace + (size_t)b * (a.iters + 1) * 8;
#pragma unroll 1
  for (int it = 0;; ++it) {              // (every branch on `it`, `done` and L.bad is uniform over the workgroup)
    fit_forward(t, a, L);
    if (tid < 8) trace[it * 8 + tid] = L.terms[tid];
    const bool last = it == a.iters;
    if (last && !(it == 0 && a.grad0)) break;
    fit_backward(t, a, L);
    if (it == 0 && a.grad0 && tid < kFitPar) a.grad0[b * kFitPar + tid] = L.g[tid];
    if (last) break;
    // Adam, torch's form: a thread per parameter; nothing is committed unless E, every gradient and every new value are finite
    b1t *= 0.9; b2t *= 0.999;
    if (tid < kFitPar) {
      const float mult = a.mult[tid < 3 ? 0 : tid < 48 ? 1 : tid < 58 ? 2 : 3];
      const float p = tid < 48 ? L.pose[tid] : tid < 58 ? L.beta[tid - 48] : L.root[tid - 58];
      const float g = L.g[tid];
      bool ok = fit_finite(g) && (tid != 0 || fit_finite(L.terms[0]));
      float c = p;
      if (mult != 0.f) {
        const float mn = L.m[tid] + (g - L.m[tid]) * 0.1f;                       // exp_avg.lerp_(grad, 1 - beta1)
        const float vn = L.v[tid] * 0.999f + (g * g) * 0.001f;                   // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
        const float step = a.lr[it] * mult / (float)(1.0 - b1t);
        const float denom = sqrtf(vn) / (float)sqrt(1.0 - b2t) + 1e-8f;
        c = p - step * (mn / denom);
        L.m_new[tid] = mn; L.v_new[tid] = vn;
        ok = ok && fit_finite(c);
      }
      L.cand[tid] = c;
      if (!ok) L.bad = 1;
    }
    __syncthreads();
    if (L.bad) { done = it; break; }
    if (tid < kFitPar && a.mult[tid < 3 ? 0 : tid < 48 ? 1 : tid < 58 ? 2 : 3] != 0.f) {
      if (tid < 48) L.pose[tid] = L.cand[tid]; else if (tid < 58) L.beta[tid - 48] = L.cand[tid]; else L.root[tid - 58] = L.cand[tid];
      L.m[tid] = L.m_new[tid]; L.v[tid] = L.v_new[tid];
    }
    __syncthreads();
  }
  // the result: the parameters (the bits they came with where nothing moved them), the count, zeros in the trace rows that were not reached
  if (tid < 48) a.pose[b * 48 + tid] = L.pose[tid];
  if (tid >= 64 && tid < 64 + kNB) a.beta[b * kNB + tid - 64] = L.beta[tid - 64];
  if (tid >= 96 && tid < 99) a.root[b * 3 + tid - 96] = L.root[tid - 96];
  if (tid == 128) a.done[b] = done;
  for (int e = (done + 1) * 8 + tid; e < (a.iters + 1) * 8; e += kFitThreads) trace[e] = 0.f;
}

}  // namespace

hipError_t launch_mano_fit(const ManoDev& t, float* pose, float* beta, float* root, const float* K, const float* kp2d, const float* conf2d,
                           const float* kp3d, const float* conf3d, const float* prior_lo, const float* prior_hi, const float* prior_w,
                           const float* lr, int iters, const float* weights6, const float* lr_mult4, int root_id, int B, float* trace,
                           float* grad0, int32_t* done, hipStream_t st) {
  FitArgs a{pose, beta, root, K, kp2d, conf2d, kp3d, conf3d, prior_lo, prior_hi, prior_w, lr, iters, root_id,
            {weights6[0], weights6[1], weights6[2], weights6[3], weights6[4], weights6[5]},
            {lr_mult4[0], lr_mult4[1], lr_mult4[2], lr_mult4[3]}, trace, grad0, done};
  hipLaunchKernelGGL(mano_fit_kernel, dim3(B), dim3(kFitThreads), 0, st, t, a);
  return hipGetLastError();
}

}  // namespace hifihr
