// Point-to-mesh distance between a point cloud and the SURFACE of a triangle mesh per sample (definition: include/hifihr.h "Point-to-mesh
// distance"): the squared distance of every point to its closest triangle and of every triangle to its closest point, with the arg-min (ties
// to the LOWEST index), the barycentric weights of the closest point, and a gradient that treats both as constants.  All arithmetic is fp64
// in one stated order (the library is built with -ffp-contract=off), so the indices, weights and minima are the integers and bits of the
// float64 restatement of tests/point_mesh_ref.py.
//   point_mesh_search_kernel       grid (direction, sample, chunk of queries).  Direction 0, points -> faces: kPointMeshPQ points per workgroup,
//                                  kPQpl per lane in registers; the faces pass through LDS in tiles of kPointMeshFT RECORDS (a, ab, ac, ab.ab,
//                                  ab.ac, ac.ac: built once per pass, not once per pair), one broadcast read of a record serves kPQpl pairs.
//                                  Direction 1, faces -> points: kPointMeshFQ faces per workgroup, kFQpl records per lane in registers (a record
//                                  is 24 VGPRs: that is what limits kFQpl), the points pass through LDS in tiles of kPointMeshPT.  Wave w scans
//                                  share w of every tile; the (d2, index) pairs of the four waves meet in LDS and are compared
//                                  lexicographically; the merging thread recomputes the winner's weights; per-chunk partial sums
//   point_mesh_finish_kernel       one workgroup folds the partial sums in a fixed order into sums[B][2] and the weighted value out[1]
//   point_mesh_bwd_points_kernel   a thread owns one point: its own term from its face, the faces that chose it as a GATHER over idx_fp
//   point_mesh_bwd_corners_kernel  a thread owns one face: the points that chose it as a GATHER over idx_pf (through LDS, ascending), its own
//                                  term, into the per-corner fp64 slab slab[B][F][3][3] of the workspace
//   point_mesh_bwd_verts_kernel    a thread owns one vertex: folds its incident corners (the host's vertex -> corner table) in ascending order
// No atomics anywhere: every output has the same bits on every call.
#include <hip/hip_runtime.h>

#include <cmath>

#include "hifihr_internal.h"

namespace hifihr {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kPQpl = kPointMeshPQ / 64;                // points a lane keeps in registers (direction 0)
constexpr int kFQpl = kPointMeshFQ / 64;                // face records a lane keeps in registers (direction 1)
constexpr int kRec = 12;                                // doubles of a face record
constexpr int kStage = kPointMeshFT * kRec;             // doubles of the staging area: a tile of records, or a tile of points
constexpr int kBwdTile = 1024;                          // entries of an index array staged per pass of a gather
constexpr int kMaxQ = kPointMeshPQ > kPointMeshFQ ? kPointMeshPQ : kPointMeshFQ;
static_assert(kPointMeshPQ <= kThreads && kPointMeshFQ <= kThreads, "the merge gives every query of a chunk one thread");
static_assert(kPointMeshPQ % 64 == 0 && kPointMeshFQ % 64 == 0, "whole waves of queries");
static_assert(kPointMeshFT % kWaves == 0 && kPointMeshPT % kWaves == 0, "equal shares of a tile");
static_assert(kPointMeshPT * 3 <= kStage, "a tile of points fits the staging area");

struct FaceRec {
  double ax, ay, az, abx, aby, abz, acx, acy, acz, abab, abac, acac;
};

__device__ __forceinline__ int clampi(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

// the record of face f of one sample's vertices: the indices are clamped into [0, V), so a foreign table cannot lead outside the array
__device__ __forceinline__ FaceRec make_rec(const float* __restrict__ v, const int* __restrict__ faces, int f, int V) {
  const int i0 = clampi(faces[(size_t)f * 3], V), i1 = clampi(faces[(size_t)f * 3 + 1], V), i2 = clampi(faces[(size_t)f * 3 + 2], V);
  FaceRec r;
  r.ax = (double)v[(size_t)i0 * 3], r.ay = (double)v[(size_t)i0 * 3 + 1], r.az = (double)v[(size_t)i0 * 3 + 2];
  r.abx = (double)v[(size_t)i1 * 3] - r.ax, r.aby = (double)v[(size_t)i1 * 3 + 1] - r.ay, r.abz = (double)v[(size_t)i1 * 3 + 2] - r.az;
  r.acx = (double)v[(size_t)i2 * 3] - r.ax, r.acy = (double)v[(size_t)i2 * 3 + 1] - r.ay, r.acz = (double)v[(size_t)i2 * 3 + 2] - r.az;
  r.abab = (r.abx * r.abx + r.aby * r.aby) + r.abz * r.abz;
  r.abac = (r.abx * r.acx + r.aby * r.acy) + r.abz * r.acz;
  r.acac = (r.acx * r.acx + r.acy * r.acy) + r.acz * r.acz;
  return r;
}

// The closest point of the triangle to p as barycentric weights, ap = p - a: the header's region form, first match wins, ONE division.
// Every comparison with a NaN is false: the chain then ends in the guarded vertex region and d2 is the NaN that never wins.
__device__ __forceinline__ void closest_weights(double apx, double apy, double apz, const FaceRec& r, double& w0, double& w1, double& w2) {
  const double d1 = (r.abx * apx + r.aby * apy) + r.abz * apz;
  const double d2 = (r.acx * apx + r.acy * apy) + r.acz * apz;
  const double d3 = d1 - r.abab, d4 = d2 - r.abac, d5 = d1 - r.abac, d6 = d2 - r.acac;
  const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
  const double e1 = d1 - d3, e2 = d2 - d6, e3a = d4 - d3, e3b = d5 - d6;
  const double e3 = e3a + e3b, den = (va + vb) + vc;
  int reg;
  if (d1 <= 0.0 && d2 <= 0.0) reg = 0;                                          // vertex a
  else if (d3 >= 0.0 && d4 <= d3) reg = 1;                                      // vertex b
  else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0 && e1 > 0.0) reg = 2;            // edge ab
  else if (d6 >= 0.0 && d5 <= d6) reg = 3;                                      // vertex c
  else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0 && e2 > 0.0) reg = 4;            // edge ac
  else if (va <= 0.0 && e3a >= 0.0 && e3b >= 0.0 && e3 > 0.0) reg = 5;          // edge bc
  else if (den > 0.0) reg = 6;                                                  // interior
  else reg = 0;                                                                 // (unreachable in exact arithmetic)
  const double num = reg == 2 ? d1 : (reg == 4 ? d2 : (reg == 5 ? e3a : (reg == 6 ? 1.0 : 0.0)));
  const double dsel = reg == 2 ? e1 : (reg == 4 ? e2 : (reg == 5 ? e3 : (reg == 6 ? den : 1.0)));
  const double q = num / dsel;                                                  // dsel > 0 in every region
  const double omq = 1.0 - q;
  const double tv = vb * q, tw = vc * q;                                        // the interior: clamped, so w0 >= 0 whatever the rounding
  const double iv = tv < 0.0 ? 0.0 : (tv > 1.0 ? 1.0 : tv);
  const double rest = 1.0 - iv;
  const double iw = tw < 0.0 ? 0.0 : (tw > rest ? rest : tw);
  w1 = reg == 1 ? 1.0 : (reg == 2 ? q : (reg == 5 ? omq : (reg == 6 ? iv : 0.0)));
  w2 = reg == 3 ? 1.0 : ((reg == 4 || reg == 5) ? q : (reg == 6 ? iw : 0.0));
  w0 = reg == 0 ? 1.0 : ((reg == 2 || reg == 4) ? omq : (reg == 6 ? rest - iw : 0.0));
}

// r = p - cp for given weights of the corners b and c: cp - a = ab w1 + ac w2
__device__ __forceinline__ void residual(double apx, double apy, double apz, const FaceRec& r, double w1, double w2, double& dx, double& dy,
                                         double& dz) {
  dx = apx - (r.abx * w1 + r.acx * w2);
  dy = apy - (r.aby * w1 + r.acy * w2);
  dz = apz - (r.abz * w1 + r.acz * w2);
}

__device__ __forceinline__ double pair_d2(double px, double py, double pz, const FaceRec& r) {
  const double apx = px - r.ax, apy = py - r.ay, apz = pz - r.az;
  double w0, w1, w2, dx, dy, dz;
  closest_weights(apx, apy, apz, r, w0, w1, w2);
  residual(apx, apy, apz, r, w1, w2, dx, dy, dz);
  return (dx * dx + dy * dy) + dz * dz;
}

__device__ __forceinline__ FaceRec rec_from_lds(const double* s, int T, int i) {
  FaceRec r;
  r.ax = s[i], r.ay = s[T + i], r.az = s[2 * T + i];
  r.abx = s[3 * T + i], r.aby = s[4 * T + i], r.abz = s[5 * T + i];
  r.acx = s[6 * T + i], r.acy = s[7 * T + i], r.acz = s[8 * T + i];
  r.abab = s[9 * T + i], r.abac = s[10 * T + i], r.acac = s[11 * T + i];
  return r;
}

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

// blockIdx.x < n_first: the direction `first`, else the other one (only when both are searched); inside a direction (b, chunk).  `first` is the
// direction whose workgroups run longest, so they are dispatched first and the short ones fill in beside them.  A direction of weight
// exactly 0 has no workgroups: none of its arrays is touched.  partial_pf[b * cpf + chunk], partial_fp[b * cfp + chunk]: the chunk's sum.
__global__ __launch_bounds__(kThreads) void point_mesh_search_kernel(const float* __restrict__ p, const float* __restrict__ v,
                                                                     const int* __restrict__ faces, int B, int N, int V, int F, int cpf, int cfp,
                                                                     int first, unsigned n_first, int* __restrict__ idx_pf,
                                                                     double* __restrict__ bary_pf, double* __restrict__ min_pf,
                                                                     int* __restrict__ idx_fp, double* __restrict__ bary_fp,
                                                                     double* __restrict__ min_fp, double* __restrict__ partial_pf,
                                                                     double* __restrict__ partial_fp) {
  __shared__ double sStage[kStage];
  __shared__ double sBest[kWaves][kMaxQ];
  __shared__ int sIdx[kWaves][kMaxQ];
  __shared__ double sRed[kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int dir = blockIdx.x < n_first ? first : 1 - first;
  const unsigned local = blockIdx.x < n_first ? blockIdx.x : blockIdx.x - n_first;
  const int chunks = dir == 0 ? cpf : cfp;
  const int b = (int)(local / (unsigned)chunks), chunk = (int)(local % (unsigned)chunks);
  const float* P = p + (size_t)b * N * 3;
  const float* Vb = v + (size_t)b * V * 3;
  double m;
  int mi;
  if (dir == 0) {
    // ---- points -> faces -------------------------------------------------------------------------------------------------------------
    const long long q0 = (long long)chunk * kPointMeshPQ;
    double qx[kPQpl], qy[kPQpl], qz[kPQpl], best[kPQpl];
    int bi[kPQpl];
#pragma unroll
    for (int k = 0; k < kPQpl; ++k) {
      const long long q = q0 + k * 64 + lane;
      const bool live = q < N;
      qx[k] = live ? (double)P[(size_t)q * 3] : 0.0;
      qy[k] = live ? (double)P[(size_t)q * 3 + 1] : 0.0;
      qz[k] = live ? (double)P[(size_t)q * 3 + 2] : 0.0;
      best[k] = INFINITY;
      bi[k] = 0;                                         // only ever replaced by a loop counter below: always in [0, F)
    }
    constexpr int kShare = kPointMeshFT / kWaves;
    for (int base = 0; base < F; base += kPointMeshFT) {
      const int cnt = F - base < kPointMeshFT ? F - base : kPointMeshFT;
      __syncthreads();
      for (int i = tid; i < cnt; i += kThreads) {
        const FaceRec r = make_rec(Vb, faces, base + i, V);
        sStage[i] = r.ax, sStage[kPointMeshFT + i] = r.ay, sStage[2 * kPointMeshFT + i] = r.az;
        sStage[3 * kPointMeshFT + i] = r.abx, sStage[4 * kPointMeshFT + i] = r.aby, sStage[5 * kPointMeshFT + i] = r.abz;
        sStage[6 * kPointMeshFT + i] = r.acx, sStage[7 * kPointMeshFT + i] = r.acy, sStage[8 * kPointMeshFT + i] = r.acz;
        sStage[9 * kPointMeshFT + i] = r.abab, sStage[10 * kPointMeshFT + i] = r.abac, sStage[11 * kPointMeshFT + i] = r.acac;
      }
      __syncthreads();
      const int lo = wave * kShare, hi = lo + kShare < cnt ? lo + kShare : cnt;
      for (int f = lo; f < hi; ++f) {
        const FaceRec r = rec_from_lds(sStage, kPointMeshFT, f);                 // one address for the wave: a broadcast
#pragma unroll
        for (int k = 0; k < kPQpl; ++k) {
          const double d2 = pair_d2(qx[k], qy[k], qz[k], r);
          // (d2, index) in lexicographic order: a wave meets its indices in ascending order, so among equals the first one stays; a
          // distance that is not a number never wins
          if (d2 < best[k]) {
            best[k] = d2;
            bi[k] = base + f;
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < kPQpl; ++k) {
      sBest[wave][k * 64 + lane] = best[k];
      sIdx[wave][k * 64 + lane] = bi[k];
    }
    __syncthreads();
    // thread t merges query t of the chunk: a wave that scanned a later share must not win a tie
    const long long q = q0 + tid;
    const bool live = tid < kPointMeshPQ && q < N;
    m = 0.0;
    mi = 0;
    if (live) {
      m = sBest[0][tid];
      mi = sIdx[0][tid];
      for (int w = 1; w < kWaves; ++w) {
        const double d = sBest[w][tid];
        const int i = sIdx[w][tid];
        if (d < m || (d == m && i < mi)) {
          m = d;
          mi = i;
        }
      }
      const FaceRec r = make_rec(Vb, faces, mi, V);
      double w0, w1, w2;
      closest_weights((double)P[(size_t)q * 3] - r.ax, (double)P[(size_t)q * 3 + 1] - r.ay, (double)P[(size_t)q * 3 + 2] - r.az, r, w0, w1, w2);
      const size_t o = (size_t)b * N + (size_t)q;
      idx_pf[o] = mi;
      min_pf[o] = m;
      bary_pf[o * 3] = w0, bary_pf[o * 3 + 1] = w1, bary_pf[o * 3 + 2] = w2;
    }
    const double s = block_sum_f64(live ? m : 0.0, sRed);
    if (tid == 0) partial_pf[(size_t)b * cpf + chunk] = s;
  } else {
    // ---- faces -> points -------------------------------------------------------------------------------------------------------------
    const long long q0 = (long long)chunk * kPointMeshFQ;
    FaceRec rec[kFQpl];
    double best[kFQpl];
    int bi[kFQpl];
#pragma unroll
    for (int k = 0; k < kFQpl; ++k) {
      const long long q = q0 + k * 64 + lane;
      rec[k] = make_rec(Vb, faces, q < F ? (int)q : F - 1, V);
      best[k] = INFINITY;
      bi[k] = 0;                                         // only ever replaced by a loop counter below: always in [0, N)
    }
    constexpr int kShare = kPointMeshPT / kWaves;
    for (int base = 0; base < N; base += kPointMeshPT) {
      const int cnt = N - base < kPointMeshPT ? N - base : kPointMeshPT;
      __syncthreads();
      for (int i = tid; i < cnt * 3; i += kThreads) sStage[i] = (double)P[(size_t)base * 3 + i];
      __syncthreads();
      const int lo = wave * kShare, hi = lo + kShare < cnt ? lo + kShare : cnt;
      for (int j = lo; j < hi; ++j) {
        const double px = sStage[j * 3], py = sStage[j * 3 + 1], pz = sStage[j * 3 + 2];     // a broadcast
#pragma unroll
        for (int k = 0; k < kFQpl; ++k) {
          const double d2 = pair_d2(px, py, pz, rec[k]);
          if (d2 < best[k]) {
            best[k] = d2;
            bi[k] = base + j;
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < kFQpl; ++k) {
      sBest[wave][k * 64 + lane] = best[k];
      sIdx[wave][k * 64 + lane] = bi[k];
    }
    __syncthreads();
    const long long q = q0 + tid;
    const bool live = tid < kPointMeshFQ && q < F;
    m = 0.0;
    mi = 0;
    if (live) {
      m = sBest[0][tid];
      mi = sIdx[0][tid];
      for (int w = 1; w < kWaves; ++w) {
        const double d = sBest[w][tid];
        const int i = sIdx[w][tid];
        if (d < m || (d == m && i < mi)) {
          m = d;
          mi = i;
        }
      }
      const FaceRec r = make_rec(Vb, faces, (int)q, V);
      double w0, w1, w2;
      closest_weights((double)P[(size_t)mi * 3] - r.ax, (double)P[(size_t)mi * 3 + 1] - r.ay, (double)P[(size_t)mi * 3 + 2] - r.az, r, w0, w1, w2);
      const size_t o = (size_t)b * F + (size_t)q;
      idx_fp[o] = mi;
      min_fp[o] = m;
      bary_fp[o * 3] = w0, bary_fp[o * 3 + 1] = w1, bary_fp[o * 3 + 2] = w2;
    }
    const double s = block_sum_f64(live ? m : 0.0, sRed);
    if (tid == 0) partial_fp[(size_t)b * cfp + chunk] = s;
  }
}

// sums[b][0] = sum_pf[b], sums[b][1] = sum_fp[b] (0 for a direction that was not searched); out[0] = w_pf mean_b(sum_pf[b] / N) +
// w_fp mean_b(sum_fp[b] / F); a weight of exactly 0 contributes exactly 0
__global__ __launch_bounds__(kThreads) void point_mesh_finish_kernel(const double* __restrict__ partial_pf, const double* __restrict__ partial_fp,
                                                                     int B, int N, int F, int cpf, int cfp, float w_pf, float w_fp,
                                                                     double* __restrict__ sums, float* __restrict__ out) {
  __shared__ double lds[2][kThreads];
  double s0 = 0.0, s1 = 0.0;
  for (int b = threadIdx.x; b < B; b += kThreads) {
    double a = 0.0, c = 0.0;
    if (w_pf != 0.f)
      for (int k = 0; k < cpf; ++k) a += partial_pf[(size_t)b * cpf + k];
    if (w_fp != 0.f)
      for (int k = 0; k < cfp; ++k) c += partial_fp[(size_t)b * cfp + k];
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
    const double vp = (w_pf != 0.f) ? (double)w_pf * (lds[0][0] / ((double)B * (double)N)) : 0.0;
    const double vf = (w_fp != 0.f) ? (double)w_fp * (lds[1][0] / ((double)B * (double)F)) : 0.0;
    out[0] = (float)(vp + vf);
  }
}

// blockIdx.x = b * chunks + chunk, a thread per point i:
//   gp[i] = gout ( c_pf r(i, a[i])  +  c_fp sum over { f : c[f] == i }, ascending, of r(i, f) ),   r(i, f) = p_i - cp with the stored weights
__global__ __launch_bounds__(kThreads) void point_mesh_bwd_points_kernel(const float* __restrict__ p, const float* __restrict__ v,
                                                                         const int* __restrict__ faces, const int* __restrict__ idx_pf,
                                                                         const double* __restrict__ bary_pf, const int* __restrict__ idx_fp,
                                                                         const double* __restrict__ bary_fp, const float* __restrict__ gout, int B,
                                                                         int N, int V, int F, int chunks, float w_pf, float w_fp,
                                                                         float* __restrict__ gp) {
  __shared__ int sI[kBwdTile];
  const int tid = threadIdx.x;
  const int b = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
  const long long i = (long long)chunk * kThreads + tid;
  const bool live = i < N;
  const float* P = p + (size_t)b * N * 3;
  const float* Vb = v + (size_t)b * V * 3;
  const double c_pf = (double)w_pf * 2.0 / ((double)B * (double)N), c_fp = (double)w_fp * 2.0 / ((double)B * (double)F);
  const double px = live ? (double)P[(size_t)i * 3] : 0.0, py = live ? (double)P[(size_t)i * 3 + 1] : 0.0,
               pz = live ? (double)P[(size_t)i * 3 + 2] : 0.0;
  double ax = 0.0, ay = 0.0, az = 0.0;
  if (w_fp != 0.f) {
    const int me = live ? (int)i : -1;                   // no index is negative: a thread past the end never hits
    const int* oth = idx_fp + (size_t)b * F;
    const double* wf = bary_fp + (size_t)b * F * 3;
    for (int base = 0; base < F; base += kBwdTile) {
      const int cnt = F - base < kBwdTile ? F - base : kBwdTile;
      __syncthreads();
      for (int j = tid; j < cnt; j += kThreads) sI[j] = oth[base + j];
      __syncthreads();
      for (int j = 0; j < cnt; ++j) {
        if (sI[j] == me) {                               // base + j is the loop counter: a face of the table whatever the array holds
          const FaceRec r = make_rec(Vb, faces, base + j, V);
          double dx, dy, dz;
          residual(px - r.ax, py - r.ay, pz - r.az, r, wf[(size_t)(base + j) * 3 + 1], wf[(size_t)(base + j) * 3 + 2], dx, dy, dz);
          ax += dx;
          ay += dy;
          az += dz;
        }
      }
    }
  }
  if (!live) return;
  double rx = 0.0, ry = 0.0, rz = 0.0;
  if (w_pf != 0.f) {
    const size_t o = (size_t)b * N + (size_t)i;
    const FaceRec r = make_rec(Vb, faces, clampi(idx_pf[o], F), V);   // the forward writes [0, F); a foreign array cannot lead outside the table
    double dx, dy, dz;
    residual(px - r.ax, py - r.ay, pz - r.az, r, bary_pf[o * 3 + 1], bary_pf[o * 3 + 2], dx, dy, dz);
    rx = c_pf * dx;
    ry = c_pf * dy;
    rz = c_pf * dz;
  }
  if (w_fp != 0.f) {
    rx += c_fp * ax;
    ry += c_fp * ay;
    rz += c_fp * az;
  }
  const double go = (double)gout[0];
  float* out = gp + ((size_t)b * N + (size_t)i) * 3;
  out[0] = (float)(go * rx);
  out[1] = (float)(go * ry);
  out[2] = (float)(go * rz);
}

// blockIdx.x = b * chunks + chunk, a thread per face f; for its corner k:
//   slab[b][f][k] = -( c_pf sum over { i : a[i] == f }, ascending, of w_k(i) r(i, f)  +  c_fp w_k(f) r(c[f], f) )
__global__ __launch_bounds__(kThreads) void point_mesh_bwd_corners_kernel(const float* __restrict__ p, const float* __restrict__ v,
                                                                          const int* __restrict__ faces, const int* __restrict__ idx_pf,
                                                                          const double* __restrict__ bary_pf, const int* __restrict__ idx_fp,
                                                                          const double* __restrict__ bary_fp, int B, int N, int V, int F,
                                                                          int chunks, float w_pf, float w_fp, double* __restrict__ slab) {
  __shared__ int sI[kBwdTile];
  const int tid = threadIdx.x;
  const int b = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
  const long long f = (long long)chunk * kThreads + tid;
  const bool live = f < F;
  const float* P = p + (size_t)b * N * 3;
  const float* Vb = v + (size_t)b * V * 3;
  const double c_pf = (double)w_pf * 2.0 / ((double)B * (double)N), c_fp = (double)w_fp * 2.0 / ((double)B * (double)F);
  const FaceRec r = make_rec(Vb, faces, live ? (int)f : F - 1, V);
  double acc[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
  if (w_pf != 0.f) {
    const int me = live ? (int)f : -1;
    const int* oth = idx_pf + (size_t)b * N;
    const double* wp = bary_pf + (size_t)b * N * 3;
    for (int base = 0; base < N; base += kBwdTile) {
      const int cnt = N - base < kBwdTile ? N - base : kBwdTile;
      __syncthreads();
      for (int j = tid; j < cnt; j += kThreads) sI[j] = oth[base + j];
      __syncthreads();
      for (int j = 0; j < cnt; ++j) {
        if (sI[j] == me) {                               // base + j is the loop counter: a point of the set whatever the array holds
          const float* q = P + (size_t)(base + j) * 3;
          const double* w = wp + (size_t)(base + j) * 3;
          double dx, dy, dz;
          residual((double)q[0] - r.ax, (double)q[1] - r.ay, (double)q[2] - r.az, r, w[1], w[2], dx, dy, dz);
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            acc[k][0] += w[k] * dx;
            acc[k][1] += w[k] * dy;
            acc[k][2] += w[k] * dz;
          }
        }
      }
    }
  }
  if (!live) return;
  double own[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
  if (w_fp != 0.f) {
    const size_t o = (size_t)b * F + (size_t)f;
    const float* q = P + (size_t)clampi(idx_fp[o], N) * 3;
    const double* w = bary_fp + o * 3;
    double dx, dy, dz;
    residual((double)q[0] - r.ax, (double)q[1] - r.ay, (double)q[2] - r.az, r, w[1], w[2], dx, dy, dz);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      own[k][0] = w[k] * dx;
      own[k][1] = w[k] * dy;
      own[k][2] = w[k] * dz;
    }
  }
  double* out = slab + ((size_t)b * F + (size_t)f) * 9;
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      double s = 0.0;
      if (w_pf != 0.f) s = c_pf * acc[k][d];
      if (w_fp != 0.f) s += c_fp * own[k][d];
      out[k * 3 + d] = -s;
    }
}

// a thread per (sample, vertex): gv[v] = gout * the sum of slab[b][corner] over the vertex's corners in the table's (ascending) order; the
// offsets and corner numbers are clamped, so a foreign table cannot lead outside the slab
__global__ __launch_bounds__(kThreads) void point_mesh_bwd_verts_kernel(const double* __restrict__ slab, const int* __restrict__ v2c_off,
                                                                        const int* __restrict__ v2c_corner, const float* __restrict__ gout, int B,
                                                                        int V, int F, int chunks, float* __restrict__ gv) {
  const int b = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
  const long long vi = (long long)chunk * kThreads + threadIdx.x;
  if (vi >= V) return;
  const long long C = (long long)F * 3;
  long long lo = v2c_off[vi], hi = v2c_off[vi + 1];
  lo = lo < 0 ? 0 : (lo > C ? C : lo);
  hi = hi < lo ? lo : (hi > C ? C : hi);
  const double* S = slab + (size_t)b * F * 9;
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (long long j = lo; j < hi; ++j) {
    long long c = v2c_corner[j];
    c = c < 0 ? 0 : (c >= C ? C - 1 : c);
    sx += S[c * 3];
    sy += S[c * 3 + 1];
    sz += S[c * 3 + 2];
  }
  const double go = (double)gout[0];
  float* out = gv + ((size_t)b * V + (size_t)vi) * 3;
  out[0] = (float)(go * sx);
  out[1] = (float)(go * sy);
  out[2] = (float)(go * sz);
}

long long point_mesh_chunks_pf(int N) { return ((long long)N + kPointMeshPQ - 1) / kPointMeshPQ; }
long long point_mesh_chunks_fp(int F) { return ((long long)F + kPointMeshFQ - 1) / kPointMeshFQ; }

bool point_mesh_grid_ok(int B, int N, int V, int F) {
  const long long lim = 0x7fffffffLL, b = B;
  const long long n = ((long long)N + kThreads - 1) / kThreads, f = ((long long)F + kThreads - 1) / kThreads,
                  vv = ((long long)V + kThreads - 1) / kThreads;
  return b * (point_mesh_chunks_pf(N) + point_mesh_chunks_fp(F)) <= lim && b * n <= lim && b * f <= lim && b * vv <= lim;
}

size_t point_mesh_partial_doubles(int B, int N, int F) { return (size_t)B * (size_t)(point_mesh_chunks_pf(N) + point_mesh_chunks_fp(F)); }

hipError_t launch_point_mesh_fwd(const float* p, const float* v, const int* faces, int B, int N, int V, int F, float w_pf, float w_fp,
                                 int* idx_pf, double* bary_pf, double* min_pf, int* idx_fp, double* bary_fp, double* min_fp, double* sums,
                                 float* out, double* ws, hipStream_t st) {
  if (B <= 0 || N < 1 || V < 1 || F < 1 || !point_mesh_grid_ok(B, N, V, F)) return hipErrorInvalidValue;
  const long long cpf = point_mesh_chunks_pf(N), cfp = point_mesh_chunks_fp(F);
  double* partial_pf = ws;
  double* partial_fp = ws + (size_t)B * cpf;
  const bool do_pf = w_pf != 0.f, do_fp = w_fp != 0.f;
  // a workgroup of direction 0 meets kPointMeshPQ * F pairs, one of direction 1 kPointMeshFQ * N: the longer ones go first
  const int first = !do_fp ? 0 : (!do_pf ? 1 : ((long long)kPointMeshPQ * F >= (long long)kPointMeshFQ * N ? 0 : 1));
  const long long n_pf = do_pf ? B * cpf : 0, n_fp = do_fp ? B * cfp : 0;
  const long long n_first = first == 0 ? n_pf : n_fp, n_second = first == 0 ? n_fp : n_pf;
  if (n_first + n_second > 0) {
    hipLaunchKernelGGL(point_mesh_search_kernel, dim3((unsigned)(n_first + n_second)), dim3(kThreads), 0, st, p, v, faces, B, N, V, F, (int)cpf,
                       (int)cfp, first, (unsigned)n_first, idx_pf, bary_pf, min_pf, idx_fp, bary_fp, min_fp, partial_pf, partial_fp);
  }
  hipLaunchKernelGGL(point_mesh_finish_kernel, dim3(1), dim3(kThreads), 0, st, partial_pf, partial_fp, B, N, F, (int)cpf, (int)cfp, w_pf, w_fp,
                     sums, out);
  return hipGetLastError();
}

hipError_t launch_point_mesh_bwd(const float* p, const float* v, const int* faces, const int* idx_pf, const double* bary_pf, const int* idx_fp,
                                 const double* bary_fp, const float* gout, const int* v2c_off, const int* v2c_corner, int B, int N, int V, int F,
                                 float w_pf, float w_fp, float* gp, float* gv, double* ws, hipStream_t st) {
  if (B <= 0 || N < 1 || V < 1 || F < 1 || !point_mesh_grid_ok(B, N, V, F)) return hipErrorInvalidValue;
  const int cn = (N + kThreads - 1) / kThreads, cf = (F + kThreads - 1) / kThreads, cv = (V + kThreads - 1) / kThreads;
  if (gp) {
    hipLaunchKernelGGL(point_mesh_bwd_points_kernel, dim3((unsigned)(B * cn)), dim3(kThreads), 0, st, p, v, faces, idx_pf, bary_pf, idx_fp,
                       bary_fp, gout, B, N, V, F, cn, w_pf, w_fp, gp);
  }
  if (gv) {
    double* slab = ws + point_mesh_partial_doubles(B, N, F);
    hipLaunchKernelGGL(point_mesh_bwd_corners_kernel, dim3((unsigned)(B * cf)), dim3(kThreads), 0, st, p, v, faces, idx_pf, bary_pf, idx_fp,
                       bary_fp, B, N, V, F, cf, w_pf, w_fp, slab);
    hipLaunchKernelGGL(point_mesh_bwd_verts_kernel, dim3((unsigned)(B * cv)), dim3(kThreads), 0, st, slab, v2c_off, v2c_corner, gout, B, V, F, cv,
                       gv);
  }
  return hipGetLastError();
}

}  // namespace hifihr
