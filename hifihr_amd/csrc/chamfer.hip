// Chamfer distance between two point sets per sample (definition: include/hifihr.h "Chamfer distance"): the squared distance of every
// point to its nearest neighbour in the other set, both directions, with the arg-min (ties to the LOWEST index) and a gradient that
// treats the arg-min as a constant.  All arithmetic is fp64 in one stated order (the library is built with -ffp-contract=off), so the
// indices and minima are the integers and bits of the float64 restatement of tests/chamfer_ref.py.
//   chamfer_search_kernel  grid (direction, sample, chunk of kChamferQ queries): the searched set passes through LDS in tiles of
//                          kChamferTile points, widened to double once; every lane keeps kQpl queries in registers, so one broadcast
//                          read of a searched point serves kQpl pairs (the loop is bound by the fp64 VALU, not by LDS reads as the
//                          one-query-per-lane fscore_counts_kernel of csrc/eval.hip is); wave w scans share w of every tile; the
//                          (d2, index) pairs of the four waves meet in LDS and are compared lexicographically; per-chunk partial sums
//   chamfer_finish_kernel  one workgroup folds the partial sums in a fixed order into sums[B][2] and the weighted value out[1]
//   chamfer_bwd_kernel     grid (set, sample, chunk of 256 points): a thread owns one point; its own term comes from its index, the
//                          scatter term is taken as a GATHER: the other set's index array passes through LDS and the thread compares
//                          every entry with its own number -- ascending order, fp64, rounded once, one writer per element
// No atomics anywhere: every output has the same bits on every call.
#include <hip/hip_runtime.h>

#include <cmath>

#include "hifihr_internal.h"

namespace hifihr {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kQpl = kChamferQ / 64;                    // queries a lane keeps in registers
constexpr int kShare = kChamferTile / kWaves;           // consecutive points of a tile that one wave scans
constexpr int kBwdTile = 1024;                          // entries of the other set's index array staged per pass
static_assert(kChamferQ == kThreads, "the merge and the backward give every thread one point");
static_assert(kChamferQ % 64 == 0 && kChamferTile % kWaves == 0, "whole waves of queries, equal shares of a tile");

// sum of one double per thread over the workgroup, in a fixed order; valid in thread 0
__device__ __forceinline__ double block_sum_f64(double v, double* lds /* [kWaves] */) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) lds[wave] = v;
  __syncthreads();
  return (lds[0] + lds[1]) + (lds[2] + lds[3]);
}

}  // namespace

// blockIdx.x = (slot * B + b) * chunks + chunk; dir 0: x searches y (idx_xy, min_xy), dir 1: y searches x.  Slot 0 is the direction with
// the LONGER searched set: its workgroups run longest (at 5990 x 778 eight times as long as the other direction's), so they are
// dispatched first and the short ones fill in beside them instead of leaving a tail of long ones at the end.
// partial[(b * 2 + dir) * chunks + chunk] = the sum of the chunk's minima; the surplus chunks of the shorter direction write nothing
// (the finisher does not read them).
__global__ __launch_bounds__(kThreads) void chamfer_search_kernel(const float* __restrict__ x, const float* __restrict__ y, int B, int N, int M,
                                                                  int chunks, int* __restrict__ idx_xy, int* __restrict__ idx_yx,
                                                                  double* __restrict__ min_xy, double* __restrict__ min_yx,
                                                                  double* __restrict__ partial) {
  __shared__ double sP[kChamferTile * 3];
  __shared__ double sBest[kWaves][kChamferQ];
  __shared__ int sIdx[kWaves][kChamferQ];
  __shared__ double sRed[kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int chunk = blockIdx.x % chunks, slot = (blockIdx.x / chunks) / B, b = (blockIdx.x / chunks) % B;
  const int dir = M >= N ? slot : 1 - slot;
  const int Nq = dir == 0 ? N : M, Ns = dir == 0 ? M : N;
  const long long q0 = (long long)chunk * kChamferQ;
  if (q0 >= Nq) return;                                  // the shorter direction has fewer chunks (uniform over the workgroup)
  const float* Q = (dir == 0 ? x : y) + (size_t)b * Nq * 3;
  const float* S = (dir == 0 ? y : x) + (size_t)b * Ns * 3;
  double qx[kQpl], qy[kQpl], qz[kQpl], best[kQpl];
  int bi[kQpl];
#pragma unroll
  for (int k = 0; k < kQpl; ++k) {
    const long long q = q0 + k * 64 + lane;
    const bool live = q < Nq;
    qx[k] = live ? (double)Q[(size_t)q * 3] : 0.0;
    qy[k] = live ? (double)Q[(size_t)q * 3 + 1] : 0.0;
    qz[k] = live ? (double)Q[(size_t)q * 3 + 2] : 0.0;
    best[k] = INFINITY;
    bi[k] = 0;                                           // only ever replaced by a loop counter below: always in [0, Ns)
  }
  for (int base = 0; base < Ns; base += kChamferTile) {
    const int cnt = Ns - base < kChamferTile ? Ns - base : kChamferTile;
    __syncthreads();
    for (int i = tid; i < cnt * 3; i += kThreads) sP[i] = (double)S[(size_t)base * 3 + i];
    __syncthreads();
    const int lo = wave * kShare, hi = lo + kShare < cnt ? lo + kShare : cnt;
    for (int p = lo; p < hi; ++p) {
      const double sx = sP[p * 3], sy = sP[p * 3 + 1], sz = sP[p * 3 + 2];      // one address for the wave: a broadcast
#pragma unroll
      for (int k = 0; k < kQpl; ++k) {
        const double dx = qx[k] - sx, dy = qy[k] - sy, dz = qz[k] - sz;
        const double d2 = (dx * dx + dy * dy) + dz * dz;
        // (d2, index) in lexicographic order: a wave meets its indices in ascending order, so among equals the first one stays; a
        // distance that is not a number never wins
        if (d2 < best[k]) {
          best[k] = d2;
          bi[k] = base + p;
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kQpl; ++k) {
    sBest[wave][k * 64 + lane] = best[k];
    sIdx[wave][k * 64 + lane] = bi[k];
  }
  __syncthreads();
  // thread t merges query t of the chunk: a wave that scanned a later share must not win a tie
  double m = sBest[0][tid];
  int mi = sIdx[0][tid];
  for (int w = 1; w < kWaves; ++w) {
    const double d = sBest[w][tid];
    const int i = sIdx[w][tid];
    if (d < m || (d == m && i < mi)) {
      m = d;
      mi = i;
    }
  }
  const long long q = q0 + tid;
  const bool live = q < Nq;
  if (live) {
    (dir == 0 ? idx_xy : idx_yx)[(size_t)b * Nq + q] = mi;
    (dir == 0 ? min_xy : min_yx)[(size_t)b * Nq + q] = m;
  }
  const double s = block_sum_f64(live ? m : 0.0, sRed);
  if (tid == 0) partial[((size_t)b * 2 + dir) * chunks + chunk] = s;
}

// sums[b][0] = sum_xy[b], sums[b][1] = sum_yx[b]; out[0] = w_xy mean_b(sum_xy[b] / N) + w_yx mean_b(sum_yx[b] / M); a weight of exactly 0
// contributes exactly 0
__global__ __launch_bounds__(kThreads) void chamfer_finish_kernel(const double* __restrict__ partial, int B, int N, int M, int chunks,
                                                                  float w_xy, float w_yx, double* __restrict__ sums,
                                                                  float* __restrict__ out) {
  __shared__ double lds[2][kThreads];
  const int cx = (N + kChamferQ - 1) / kChamferQ, cy = (M + kChamferQ - 1) / kChamferQ;
  double s0 = 0.0, s1 = 0.0;
  for (int b = threadIdx.x; b < B; b += kThreads) {
    const double* p = partial + (size_t)b * 2 * chunks;
    double a = 0.0, c = 0.0;
    for (int k = 0; k < cx; ++k) a += p[k];
    for (int k = 0; k < cy; ++k) c += p[chunks + k];
    sums[2 * (size_t)b] = a;
    sums[2 * (size_t)b + 1] = c;
    s0 += a;
    s1 += c;
  }
  lds[0][threadIdx.x] = s0;
  lds[1][threadIdx.x] = s1;
  __syncthreads();
  for (int w = kThreads / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      lds[0][threadIdx.x] += lds[0][threadIdx.x + w];
      lds[1][threadIdx.x] += lds[1][threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double vx = (w_xy != 0.f) ? (double)w_xy * (lds[0][0] / ((double)B * (double)N)) : 0.0;
    const double vy = (w_yx != 0.f) ? (double)w_yx * (lds[1][0] / ((double)B * (double)M)) : 0.0;
    out[0] = (float)(vx + vy);
  }
}

// blockIdx.x = (slot * B + b) * chunks + chunk, slot 0 = the set that gathers over the longer index array; set 0 writes gx (the points of
// x), set 1 writes gy.  For the point i of its set:
//   g[i] = gout ( c_own (p_i - o[own[i]])  +  c_oth sum over { j : oth[j] == i }, ascending, of (p_i - o_j) )
// own = the index array of the set's own direction, oth = the other direction's; a direction of weight exactly 0 is skipped.
__global__ __launch_bounds__(kThreads) void chamfer_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                               const int* __restrict__ idx_xy, const int* __restrict__ idx_yx,
                                                               const float* __restrict__ gout, int B, int N, int M, int chunks, float w_xy,
                                                               float w_yx, float* __restrict__ gx, float* __restrict__ gy) {
  __shared__ int sI[kBwdTile];
  const int tid = threadIdx.x;
  const int chunk = blockIdx.x % chunks, slot = (blockIdx.x / chunks) / B, b = (blockIdx.x / chunks) % B;
  const int set = M >= N ? slot : 1 - slot;
  float* g = set == 0 ? gx : gy;
  if (g == nullptr) return;                              // (uniform over the workgroup)
  const int Np = set == 0 ? N : M, No = set == 0 ? M : N;
  const long long i = (long long)chunk * kThreads + tid;
  if ((long long)chunk * kThreads >= Np) return;
  const float* P = (set == 0 ? x : y) + (size_t)b * Np * 3;
  const float* O = (set == 0 ? y : x) + (size_t)b * No * 3;
  const int* own = (set == 0 ? idx_xy : idx_yx) + (size_t)b * Np;
  const int* oth = (set == 0 ? idx_yx : idx_xy) + (size_t)b * No;
  const float w_own = set == 0 ? w_xy : w_yx, w_oth = set == 0 ? w_yx : w_xy;
  const double c_own = (double)w_own * 2.0 / ((double)B * (double)Np), c_oth = (double)w_oth * 2.0 / ((double)B * (double)No);
  const bool live = i < Np;
  const double px = live ? (double)P[(size_t)i * 3] : 0.0, py = live ? (double)P[(size_t)i * 3 + 1] : 0.0,
               pz = live ? (double)P[(size_t)i * 3 + 2] : 0.0;
  double ax = 0.0, ay = 0.0, az = 0.0;
  if (w_oth != 0.f) {
    const int me = live ? (int)i : -1;                   // no index is negative: a thread past the end never hits
    for (int base = 0; base < No; base += kBwdTile) {
      const int cnt = No - base < kBwdTile ? No - base : kBwdTile;
      __syncthreads();
      for (int j = tid; j < cnt; j += kThreads) sI[j] = oth[base + j];
      __syncthreads();
      for (int j = 0; j < cnt; ++j) {
        if (sI[j] == me) {                               // j is the loop counter: o_j is inside the set whatever the array holds
          const float* o = O + (size_t)(base + j) * 3;
          ax += px - (double)o[0];
          ay += py - (double)o[1];
          az += pz - (double)o[2];
        }
      }
    }
  }
  if (!live) return;
  double rx = 0.0, ry = 0.0, rz = 0.0;
  if (w_own != 0.f) {
    int a = own[i];
    a = a < 0 ? 0 : (a >= No ? No - 1 : a);              // the forward writes [0, No); a foreign array cannot lead outside the set
    const float* o = O + (size_t)a * 3;
    rx = c_own * (px - (double)o[0]);
    ry = c_own * (py - (double)o[1]);
    rz = c_own * (pz - (double)o[2]);
  }
  if (w_oth != 0.f) {
    rx += c_oth * ax;
    ry += c_oth * ay;
    rz += c_oth * az;
  }
  const double go = (double)gout[0];
  float* out = g + ((size_t)b * Np + (size_t)i) * 3;
  out[0] = (float)(go * rx);
  out[1] = (float)(go * ry);
  out[2] = (float)(go * rz);
}

long long chamfer_chunks(int N, int M) {
  const long long n = N > M ? N : M;
  return (n + kChamferQ - 1) / kChamferQ;
}

hipError_t launch_chamfer_fwd(const float* x, const float* y, int B, int N, int M, float w_xy, float w_yx, int* idx_xy, int* idx_yx,
                              double* min_xy, double* min_yx, double* sums, float* out, double* partial, hipStream_t st) {
  const long long chunks = chamfer_chunks(N, M);
  if (B <= 0 || N < 1 || M < 1 || (long long)B * 2 * chunks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(chamfer_search_kernel, dim3((unsigned)(B * 2 * chunks)), dim3(kThreads), 0, st, x, y, B, N, M, (int)chunks, idx_xy, idx_yx,
                     min_xy, min_yx, partial);
  hipLaunchKernelGGL(chamfer_finish_kernel, dim3(1), dim3(kThreads), 0, st, partial, B, N, M, (int)chunks, w_xy, w_yx, sums, out);
  return hipGetLastError();
}

hipError_t launch_chamfer_bwd(const float* x, const float* y, const int* idx_xy, const int* idx_yx, const float* gout, int B, int N, int M,
                              float w_xy, float w_yx, float* gx, float* gy, hipStream_t st) {
  const long long chunks = chamfer_chunks(N, M);
  if (B <= 0 || N < 1 || M < 1 || (long long)B * 2 * chunks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(chamfer_bwd_kernel, dim3((unsigned)(B * 2 * chunks)), dim3(kThreads), 0, st, x, y, idx_xy, idx_yx, gout, B, N, M,
                     (int)chunks, w_xy, w_yx, gx, gy);
  return hipGetLastError();
}

}  // namespace hifihr
