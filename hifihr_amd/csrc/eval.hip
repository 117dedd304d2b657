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

}  // namespace hifihr
