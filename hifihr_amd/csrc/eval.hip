// Evaluation path: Procrustes-with-scale alignment of a predicted point set to its ground truth and
// the aligned per-point error, batched -- one workgroup per sample, no host round trip.
//
// Replaces the per-sample numpy loop of reference train_hrnet.py:227-243 around utils/train_utils.py:267-290 (align_w_scale:
// centre, Frobenius-normalise, scipy.linalg.orthogonal_procrustes, apply).  With A = (gt - mean)/s1 and B = (pred - mean)/s2
// (s = Frobenius norm + 1e-8), scipy takes  u w v^T = svd(A^T B),  R = u v^T,  scale = sum(w)  -- no determinant
// correction, a reflection is allowed -- and the aligned prediction is  (B R^T) scale s1 + mean(gt).
// R is the orthogonal polar factor of M = A^T B and scale = sum(w); both come from a one-sided Jacobi SVD of the 3x3 M (polar3 below),
// which also completes R where M is rank-deficient (coplanar / collinear points), as scipy's full SVD does.  All of it in fp64 (numpy does the same on
// fp64 arrays); the points are read as fp32, 12 bytes per point per set: the kernel is HBM / latency bound and tiny.
#include <hip/hip_runtime.h>

#include <cmath>

#include "hifihr_internal.h"

namespace hifihr {

namespace {

constexpr int kThreads = 256;

// sum of `v` over the workgroup, result to every thread
__device__ double block_sum(double v, double* red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  return red[0];
}

// Orthogonal polar factor R = U V^T and scale = sum of the singular values of a 3x3 M = U diag(w) V^T, from a one-sided (Hestenes) Jacobi
// SVD of M itself: right rotations make the columns of W = M V orthogonal, their lengths are w.  Working on M -- not on M^T M -- keeps
// the condition number unsquared, so a singular value of 1e-8 of the largest still has its direction to fp64 rounding.  The third left
// vector is never taken from a (possibly vanishing) column: it is +-(u1 x u2), the sign read off the column where that column is
// above rounding.  Rank-deficient M (LAPACK returns SOME orthonormal completion there, scipy takes it): the missing directions are
// completed to the proper rotation, det R = +1; see include/hifihr.h for what is and is not unique then.
__device__ void polar3(const double M[3][3], double R[3][3], double* scale) {
  double W[3][3], V[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) { W[i][j] = M[i][j]; V[i][j] = i == j ? 1.0 : 0.0; }
  for (int sweep = 0; sweep < 40; ++sweep) {
    bool rotated = false;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        double al = 0.0, be = 0.0, ga = 0.0;
        for (int k = 0; k < 3; ++k) { al += W[k][p] * W[k][p]; be += W[k][q] * W[k][q]; ga += W[k][p] * W[k][q]; }
        if (ga == 0.0 || fabs(ga) <= 2.3e-16 * sqrt(al) * sqrt(be)) continue;
        rotated = true;
        const double zeta = (be - al) / (2.0 * ga);
        const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(zeta * zeta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 3; ++k) {
          const double a = W[k][p], b = W[k][q];
          W[k][p] = c * a - s * b; W[k][q] = s * a + c * b;
          const double e = V[k][p], f = V[k][q];
          V[k][p] = c * e - s * f; V[k][q] = s * e + c * f;
        }
      }
    if (!rotated) break;
  }
  double w[3];
  int o[3] = {0, 1, 2};
  for (int k = 0; k < 3; ++k) w[k] = sqrt(W[0][k] * W[0][k] + W[1][k] * W[1][k] + W[2][k] * W[2][k]);
  for (int i = 0; i < 2; ++i)                       // descending order of w
    for (int j = 0; j < 2 - i; ++j)
      if (w[o[j]] < w[o[j + 1]]) { const int tmp = o[j]; o[j] = o[j + 1]; o[j + 1] = tmp; }
  *scale = w[0] + w[1] + w[2];
  const double w1 = w[o[0]], w2 = w[o[1]], w3 = w[o[2]];
  const double kRank = 1e-14;                        // a column below this fraction of the largest is rounding of the sums that made M
  double u[3][3], v[3][3];                           // [k][.]: k-th left / right singular vector
  for (int k = 0; k < 3; ++k)
    for (int i = 0; i < 3; ++i) v[k][i] = V[i][o[k]];
  if (!(w1 > 0.0)) {                                 // M = 0 (a set that is a single point): scale = 0, any R serves
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) R[i][j] = i == j ? 1.0 : 0.0;
    return;
  }
  for (int i = 0; i < 3; ++i) u[0][i] = W[i][o[0]] / w1;
  double n2 = 0.0;
  if (w2 > kRank * w1) {                             // u2: the second column, re-orthogonalised against u1
    double d = 0.0;
    for (int i = 0; i < 3; ++i) d += W[i][o[1]] * u[0][i];
    for (int i = 0; i < 3; ++i) { u[1][i] = W[i][o[1]] - d * u[0][i]; n2 += u[1][i] * u[1][i]; }
  }
  if (!(w2 > kRank * w1) || !(n2 > 0.0)) {           // rank 1: any unit vector orthogonal to u1 (the axis u1 is smallest along)
    int m = 0;
    for (int i = 1; i < 3; ++i) if (fabs(u[0][i]) < fabs(u[0][m])) m = i;
    n2 = 0.0;
    for (int i = 0; i < 3; ++i) { u[1][i] = (i == m ? 1.0 : 0.0) - u[0][m] * u[0][i]; n2 += u[1][i] * u[1][i]; }
  }
  n2 = sqrt(n2);
  for (int i = 0; i < 3; ++i) u[1][i] /= n2;
  u[2][0] = u[0][1] * u[1][2] - u[0][2] * u[1][1];
  u[2][1] = u[0][2] * u[1][0] - u[0][0] * u[1][2];
  u[2][2] = u[0][0] * u[1][1] - u[0][1] * u[1][0];
  double sgn;
  if (w3 > kRank * w1 && w2 > kRank * w1) {          // the data decide between the rotation and the reflection
    sgn = (W[0][o[2]] * u[2][0] + W[1][o[2]] * u[2][1] + W[2][o[2]] * u[2][2]) >= 0.0 ? 1.0 : -1.0;
  } else {                                           // they do not: det U = det V, the proper rotation
    const double detv = v[0][0] * (v[1][1] * v[2][2] - v[1][2] * v[2][1]) - v[0][1] * (v[1][0] * v[2][2] - v[1][2] * v[2][0]) +
                        v[0][2] * (v[1][0] * v[2][1] - v[1][1] * v[2][0]);
    sgn = detv >= 0.0 ? 1.0 : -1.0;
  }
  for (int i = 0; i < 3; ++i) u[2][i] *= sgn;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) R[i][j] = u[0][i] * v[0][j] + u[1][i] * v[1][j] + u[2][i] * v[2][j];
}

}  // namespace

__global__ __launch_bounds__(kThreads) void procrustes_kernel(const float* __restrict__ pred, const float* __restrict__ gt, int N,
                                                             float* __restrict__ aligned, float* __restrict__ err_sum) {
  __shared__ double red[kThreads];
  __shared__ double sR[9], sScale;
  const int b = blockIdx.x;
  const float* P = pred + (size_t)b * N * 3;
  const float* G = gt + (size_t)b * N * 3;
  // pass 1: means
  double a[6] = {0, 0, 0, 0, 0, 0};
  for (int n = threadIdx.x; n < N; n += kThreads)
    for (int k = 0; k < 3; ++k) { a[k] += (double)G[n * 3 + k]; a[3 + k] += (double)P[n * 3 + k]; }
  double t1[3], t2[3];
  for (int k = 0; k < 3; ++k) { t1[k] = block_sum(a[k], red) / N; t2[k] = block_sum(a[3 + k], red) / N; }
  // pass 2: Frobenius norms and the cross-covariance of the centred sets
  double m[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, n1 = 0.0, n2 = 0.0;
  for (int n = threadIdx.x; n < N; n += kThreads) {
    double g[3], p[3];
    for (int k = 0; k < 3; ++k) { g[k] = (double)G[n * 3 + k] - t1[k]; p[k] = (double)P[n * 3 + k] - t2[k]; }
    for (int i = 0; i < 3; ++i) {
      n1 += g[i] * g[i]; n2 += p[i] * p[i];
      for (int j = 0; j < 3; ++j) m[i * 3 + j] += g[i] * p[j];
    }
  }
  n1 = block_sum(n1, red); n2 = block_sum(n2, red);
  for (int k = 0; k < 9; ++k) m[k] = block_sum(m[k], red);
  const double s1 = sqrt(n1) + 1e-8, s2 = sqrt(n2) + 1e-8;
  if (threadIdx.x == 0) {
    double M[3][3], R[3][3], scale;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) M[i][j] = m[i * 3 + j] / (s1 * s2);          // A^T B
    polar3(M, R, &scale);
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) sR[i * 3 + j] = R[i][j];
    sScale = scale;
  }
  __syncthreads();
  // pass 3: aligned_n = R ((pred_n - t2) / s2) * scale * s1 + t1, error against gt_n
  const double f = sScale * s1 / s2;
  double e = 0.0;
  for (int n = threadIdx.x; n < N; n += kThreads) {
    double p[3], d2 = 0.0;
    for (int k = 0; k < 3; ++k) p[k] = (double)P[n * 3 + k] - t2[k];
    for (int i = 0; i < 3; ++i) {
      const double v = (sR[i * 3] * p[0] + sR[i * 3 + 1] * p[1] + sR[i * 3 + 2] * p[2]) * f + t1[i];
      if (aligned != nullptr) aligned[((size_t)b * N + n) * 3 + i] = (float)v;
      const double d = v - (double)G[n * 3 + i];
      d2 += d * d;
    }
    e += sqrt(d2);
  }
  e = block_sum(e, red);
  if (threadIdx.x == 0) err_sum[b] = (float)e;
}

hipError_t launch_procrustes(const float* pred, const float* gt, int B, int N, float* aligned, float* err_sum, hipStream_t st) {
  if (B <= 0 || N <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(procrustes_kernel, dim3(B), dim3(kThreads), 0, st, pred, gt, N, aligned, err_sum);
  return hipGetLastError();
}

// ---- benchmark metrics: the counts behind the FreiHAND benchmark's PCK / AUC and F-score (reference utils/fh_utils.py:719-815
// EvalUtil; the benchmark's calculate_fscore).  The device counts, the host (hifihr_amd/evaluate.py) turns counts into curves.

namespace {

constexpr int kHistKp = 4;            // adjacent keypoints per workgroup: 48 contiguous bytes of every sample row
static_assert(kThreads % kHistKp == 0 && (kHistKp & (kHistKp - 1)) == 0, "a thread keeps one keypoint; the tree sum keeps the classes apart");
constexpr int kFsQ = 64;              // queries per workgroup: one per lane, every wave searches a quarter of each tile
constexpr int kFsWaves = kThreads / 64;
constexpr int kFsTile = 512;          // searched points staged per pass, as doubles: 12 KiB of LDS
static_assert(kFsTile % kFsWaves == 0, "every wave takes the same share of a tile");

}  // namespace

// One workgroup per kHistKp adjacent keypoints; thread t keeps keypoint t % kHistKp and walks the samples t / kHistKp, + kThreads / kHistKp, ...
// The bins are LDS integers (atomic adds of integers: the same bits in any order), the distance sum is a per-thread chain then a fixed tree.
__global__ __launch_bounds__(kThreads) void point_error_hist_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                                   const unsigned char* __restrict__ vis, int n, int K, HistThresholds thr,
                                                                   int T, int* __restrict__ hist, double* __restrict__ sum) {
  __shared__ double red[kThreads];
  __shared__ double sThr[kHistMaxT];
  __shared__ int sBin[kHistKp * (kHistMaxT + 1)];
  const int tid = threadIdx.x, j = tid % kHistKp, k0 = blockIdx.x * kHistKp, k = k0 + j;
  for (int i = tid; i < kHistKp * (T + 1); i += kThreads) sBin[i] = 0;
  for (int t = tid; t < T; t += kThreads) sThr[t] = thr.v[t];
  __syncthreads();
  double acc = 0.0;
  if (k < K)
    for (int s = tid / kHistKp; s < n; s += kThreads / kHistKp) {
      const size_t at = (size_t)s * K + k;
      if (vis != nullptr && vis[at] == 0) continue;
      const double dx = (double)pred[at * 3] - (double)gt[at * 3], dy = (double)pred[at * 3 + 1] - (double)gt[at * 3 + 1],
                   dz = (double)pred[at * 3 + 2] - (double)gt[at * 3 + 2];
      const double d = sqrt(dx * dx + dy * dy + dz * dz);
      int lo = 0, hi = T;                                // first t with d <= thr[t]; T when there is none (d beyond the last, or not a number)
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (d <= sThr[mid]) hi = mid; else lo = mid + 1;
      }
      atomicAdd(&sBin[j * (T + 1) + lo], 1);
      acc += d;
    }
  red[tid] = acc;
  __syncthreads();
  for (int s = kThreads / 2; s >= kHistKp; s >>= 1) {    // s is a multiple of kHistKp: a keypoint's partial sums only meet each other
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid < kHistKp && k0 + tid < K) sum[k0 + tid] = red[tid];
  for (int i = tid; i < kHistKp * (T + 1); i += kThreads)
    if (k0 + i / (T + 1) < K) hist[(size_t)k0 * (T + 1) + i] = sBin[i];
}

// Nearest neighbour of kFsQ queries in the other set of their sample, both directions in one launch: blockIdx.x = (sample, direction, chunk).
// The searched set passes through LDS in tiles of kFsTile points (widened to double once); lane l of every wave keeps query l and
// scans its wave's share of the tile -- all lanes read the same LDS address, a broadcast --, the four partial minima meet in LDS.
// min d^2 does not depend on the order of the search, the counts are integer atomics: the same bits on every call.
__global__ __launch_bounds__(kThreads) void fscore_counts_kernel(const float* __restrict__ pred, const float* __restrict__ gt, int Np, int Ng,
                                                                int chunks, FscoreThresholds thr, int T, int* __restrict__ counts) {
  __shared__ double sP[kFsTile * 3];
  __shared__ double sMin[kFsWaves][kFsQ];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int chunk = blockIdx.x % chunks, dir = (blockIdx.x / chunks) & 1, b = blockIdx.x / (2 * chunks);
  const int Nq = dir == 0 ? Np : Ng, Ns = dir == 0 ? Ng : Np;
  if (chunk * kFsQ >= Nq) return;                        // the shorter direction has fewer chunks (uniform over the workgroup)
  const float* Q = (dir == 0 ? pred : gt) + (size_t)b * Nq * 3;
  const float* S = (dir == 0 ? gt : pred) + (size_t)b * Ns * 3;
  const int q = chunk * kFsQ + lane;
  const bool live = q < Nq;
  const double qx = live ? (double)Q[(size_t)q * 3] : 0.0, qy = live ? (double)Q[(size_t)q * 3 + 1] : 0.0,
               qz = live ? (double)Q[(size_t)q * 3 + 2] : 0.0;
  double best = INFINITY;
  for (int base = 0; base < Ns; base += kFsTile) {
    const int cnt = Ns - base < kFsTile ? Ns - base : kFsTile;
    __syncthreads();
    for (int i = tid; i < cnt * 3; i += kThreads) sP[i] = (double)S[(size_t)base * 3 + i];
    __syncthreads();
    const int per = kFsTile / kFsWaves, lo = wave * per, hi = lo + per < cnt ? lo + per : cnt;
    for (int p = lo; p < hi; ++p) {
      const double dx = qx - sP[p * 3], dy = qy - sP[p * 3 + 1], dz = qz - sP[p * 3 + 2];
      const double d2 = dx * dx + dy * dy + dz * dz;
      best = d2 < best ? d2 : best;                      // a distance that is not a number never wins
    }
  }
  sMin[wave][lane] = best;
  __syncthreads();
  if (wave != 0) return;
  for (int w = 1; w < kFsWaves; ++w) best = sMin[w][lane] < best ? sMin[w][lane] : best;
  const double d = sqrt(best);
  for (int t = 0; t < T; ++t) {
    const unsigned long long m = __ballot(live && d < thr.v[t]);
    if (lane == 0 && m != 0ull) atomicAdd(&counts[((size_t)b * 2 + dir) * T + t], __popcll(m));
  }
}

bool thresholds_ok(const double* thr, int T, bool positive) {
  if (thr == nullptr || T <= 0) return false;
  for (int t = 0; t < T; ++t) {
    if (!std::isfinite(thr[t])) return false;
    if (positive ? !(thr[t] > 0.0) : (t > 0 && !(thr[t] > thr[t - 1]))) return false;
  }
  return true;
}

hipError_t launch_point_error_hist(const float* pred, const float* gt, const unsigned char* vis, int n, int K, const double* thr_h, int T,
                                   int* hist, double* sum, hipStream_t st) {
  if (n <= 0 || K <= 0 || T > kHistMaxT || !thresholds_ok(thr_h, T, false)) return hipErrorInvalidValue;
  HistThresholds thr;
  for (int t = 0; t < kHistMaxT; ++t) thr.v[t] = t < T ? thr_h[t] : 0.0;
  hipLaunchKernelGGL(point_error_hist_kernel, dim3((K + kHistKp - 1) / kHistKp), dim3(kThreads), 0, st, pred, gt, vis, n, K, thr, T, hist, sum);
  return hipGetLastError();
}

hipError_t launch_fscore_counts(const float* pred, const float* gt, int B, int Np, int Ng, const double* thr_h, int T, int* counts,
                                hipStream_t st) {
  if (B <= 0 || Np <= 0 || Ng <= 0 || T > kFscoreMaxT || !thresholds_ok(thr_h, T, true)) return hipErrorInvalidValue;
  const int chunks = ((Np > Ng ? Np : Ng) + kFsQ - 1) / kFsQ;
  if ((long long)B * 2 * chunks > 0x7fffffffLL) return hipErrorInvalidValue;
  FscoreThresholds thr;
  for (int t = 0; t < kFscoreMaxT; ++t) thr.v[t] = t < T ? thr_h[t] : 0.0;
  hipError_t e = hipMemsetAsync(counts, 0, sizeof(int) * (size_t)B * 2 * T, st);      // the workgroups of a sample add into its row
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(fscore_counts_kernel, dim3((unsigned)(B * 2 * chunks)), dim3(kThreads), 0, st, pred, gt, Np, Ng, chunks, thr, T, counts);
  return hipGetLastError();
}

}  // namespace hifihr
