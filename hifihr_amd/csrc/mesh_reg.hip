// Two mesh regularisers in one kernel pair (definitions: include/hifihr.h "Mesh regularisers"):
//   triangle            lam_lap * mean over (sample, vertex) of || mean of the neighbours - vertex ||      (the reference's
//                       losses.py:421-429: lambda_laplacian * mesh_laplacian_smoothing(Meshes(verts, faces), method="uniform"))
//   normal_consistency  lam_nc * mean over (sample, quad) of 1 - cos(angle between the normals of two faces on one edge)
//                       (PyTorch3D's mesh_normal_consistency; not in the reference)
// Every index comes from the tables hifihr_mesh_topology_create built and checked on the host (csrc/hifihr_api.hip): the neighbour
// list in compressed-row form, the quad records (v0, v1, a, b) and the vertex -> (quad * 4 + role) list.
//   mesh_reg_fwd_kernel     grid (B, ceil(max(V, Q) / 256)): a thread takes one vertex (d_i, its norm, unit_d = d_i / |d_i|) and one quad
//                           (1 - cos); per-workgroup partial sums
//   mesh_reg_finish_kernel  one workgroup folds the partial sums in a fixed order, in double, into out[2]
//   mesh_reg_bwd_kernel     grid (B, ceil(V / 256)): vertex k gathers unit_d of its neighbours and recomputes the gradient of every
//                           quad it belongs to; one writer per element, overwritten
// No atomics anywhere: out, unit_d and gverts have the same bits on every call.
#include <hip/hip_runtime.h>

#include "hifihr_internal.h"

namespace hifihr {

namespace {

constexpr float kCosEps = 1e-8f;      // the clamp of F.cosine_similarity(eps=1e-8)

struct M3 {
  float x, y, z;
};
__device__ __forceinline__ M3 m_ld(const float* __restrict__ v, int i) { return {v[3 * i], v[3 * i + 1], v[3 * i + 2]}; }
__device__ __forceinline__ M3 m_sub(M3 a, M3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ M3 m_cross(M3 a, M3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ float m_dot(M3 a, M3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ float m_norm(M3 a) { return sqrtf(m_dot(a, a)); }

// the two normals of a quad record: n0 = e x (a - v0), n1 = -(e x (b - v0)), e = v1 - v0
struct QuadGeom {
  M3 e, p0, p1, n0, n1;
  float l0, l1;
};
__device__ __forceinline__ QuadGeom quad_geom(const float* __restrict__ v, const int* __restrict__ rec) {
  QuadGeom g;
  const M3 v0 = m_ld(v, rec[0]);
  g.e = m_sub(m_ld(v, rec[1]), v0);
  g.p0 = m_sub(m_ld(v, rec[2]), v0);
  g.p1 = m_sub(m_ld(v, rec[3]), v0);
  g.n0 = m_cross(g.e, g.p0);
  const M3 m = m_cross(g.e, g.p1);
  g.n1 = {-m.x, -m.y, -m.z};
  g.l0 = m_norm(g.n0);
  g.l1 = m_norm(g.n1);
  return g;
}

// sum of one double per thread over the 256 threads of the workgroup, in a fixed order; valid in thread 0
__device__ __forceinline__ double block_sum_f64(double v, double* lds /* [4] */) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) lds[wave] = v;
  __syncthreads();
  return (lds[0] + lds[1]) + (lds[2] + lds[3]);
}

}  // namespace

// partial[(b * gridDim.y + blockIdx.y) * 2 + {0, 1}] = (sum of |d_i|, sum of 1 - cos) over the workgroup's vertices / quads
__global__ __launch_bounds__(256) void mesh_reg_fwd_kernel(MeshTopoDev t, const float* __restrict__ verts, int do_lap, int do_nc,
                                                          float* __restrict__ unit, float* __restrict__ partial) {
  __shared__ double lds[2][4];
  const int b = blockIdx.x;
  const float* v = verts + (size_t)b * t.V * 3;
  float* u = unit + (size_t)b * t.V * 3;
  double s_lap = 0.0, s_nc = 0.0;
  for (int i = blockIdx.y * 256 + threadIdx.x; i < t.V; i += 256 * gridDim.y) {
    M3 un = {0.f, 0.f, 0.f};
    if (do_lap) {
      M3 s = {0.f, 0.f, 0.f};
      for (int e = t.nbr_off[i]; e < t.nbr_off[i + 1]; ++e) {          // ascending neighbour index: a fixed order
        const M3 w = m_ld(v, t.nbr_idx[e]);
        s.x += w.x; s.y += w.y; s.z += w.z;
      }
      const float r = t.deg[i];                                         // a vertex without a neighbour: the sum is 0 and d = -v
      if (r > 0.f) s = {s.x / r, s.y / r, s.z / r};                     // a division: the mean of equal-and-opposite offsets is exact
      const M3 vi = m_ld(v, i);
      const M3 d = {s.x - vi.x, s.y - vi.y, s.z - vi.z};
      const float l = m_norm(d);
      if (l > 0.f) un = {d.x / l, d.y / l, d.z / l};                    // the subgradient at d = 0 is 0
      s_lap += (double)l;
    }
    u[3 * i] = un.x; u[3 * i + 1] = un.y; u[3 * i + 2] = un.z;
  }
  if (do_nc) {
    for (int q = blockIdx.y * 256 + threadIdx.x; q < t.Q; q += 256 * gridDim.y) {
      const QuadGeom g = quad_geom(v, t.quads + 4 * (size_t)q);
      const float c = m_dot(g.n0, g.n1) / (fmaxf(g.l0, kCosEps) * fmaxf(g.l1, kCosEps));
      s_nc += (double)(1.f - c);
    }
  }
  s_lap = block_sum_f64(s_lap, lds[0]);
  s_nc = block_sum_f64(s_nc, lds[1]);
  if (threadIdx.x == 0) {
    float* p = partial + ((size_t)b * gridDim.y + blockIdx.y) * 2;
    p[0] = (float)s_lap;
    p[1] = (float)s_nc;
  }
}

// out[0] = lam_lap * sum partial[.][0] / (B V), out[1] = lam_nc * sum partial[.][1] / (B Q) (0 when Q == 0); a weight of exactly 0 gives 0
__global__ __launch_bounds__(256) void mesh_reg_finish_kernel(MeshTopoDev t, const float* __restrict__ partial, long n, int B, float lam_lap,
                                                             float lam_nc, float* __restrict__ out) {
  __shared__ double lds[2][256];
  double s0 = 0.0, s1 = 0.0;
  for (long i = threadIdx.x; i < n; i += 256) {
    s0 += (double)partial[2 * i];
    s1 += (double)partial[2 * i + 1];
  }
  lds[0][threadIdx.x] = s0;
  lds[1][threadIdx.x] = s1;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      lds[0][threadIdx.x] += lds[0][threadIdx.x + w];
      lds[1][threadIdx.x] += lds[1][threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = (lam_lap != 0.f) ? (float)((double)lam_lap * lds[0][0] / ((double)B * t.V)) : 0.f;
    out[1] = (lam_nc != 0.f && t.Q > 0) ? (float)((double)lam_nc * lds[1][0] / ((double)B * t.Q)) : 0.f;
  }
}

// gout[2]: the gradients of the two (already weighted) terms.  gverts[b][k] = c_lap (-u_k + sum over i in N(k) of u_i / deg(i))
//   + c_nc sum over the (quad, role) entries of k of d(1 - cos) / d(that corner).
__global__ __launch_bounds__(256) void mesh_reg_bwd_kernel(MeshTopoDev t, const float* __restrict__ verts, const float* __restrict__ unit,
                                                          const float* __restrict__ gout, int B, float lam_lap, float lam_nc,
                                                          float* __restrict__ gverts) {
  const int b = blockIdx.x;
  const float* v = verts + (size_t)b * t.V * 3;
  const float* u = unit + (size_t)b * t.V * 3;
  float* gv = gverts + (size_t)b * t.V * 3;
  const float c_lap = (lam_lap != 0.f) ? gout[0] * lam_lap / ((float)B * (float)t.V) : 0.f;
  const float c_nc = (lam_nc != 0.f && t.Q > 0) ? gout[1] * lam_nc / ((float)B * (float)t.Q) : 0.f;
  for (int k = blockIdx.y * 256 + threadIdx.x; k < t.V; k += 256 * gridDim.y) {
    M3 g = {0.f, 0.f, 0.f};
    if (lam_lap != 0.f) {
      M3 s = {0.f, 0.f, 0.f};
      for (int e = t.nbr_off[k]; e < t.nbr_off[k + 1]; ++e) {
        const int i = t.nbr_idx[e];
        const M3 ui = m_ld(u, i);
        const float r = t.deg[i];                                       // >= 1: i has the neighbour k
        s.x += ui.x / r; s.y += ui.y / r; s.z += ui.z / r;
      }
      const M3 uk = m_ld(u, k);
      g = {c_lap * (s.x - uk.x), c_lap * (s.y - uk.y), c_lap * (s.z - uk.z)};
    }
    if (lam_nc != 0.f) {
      M3 a = {0.f, 0.f, 0.f};
      for (int e = t.vq_off[k]; e < t.vq_off[k + 1]; ++e) {             // ascending quad order: a fixed order
        const int q = t.vq_idx[e] >> 2, role = t.vq_idx[e] & 3;
        const QuadGeom qg = quad_geom(v, t.quads + 4 * (size_t)q);
        if (!(qg.l0 > kCosEps && qg.l1 > kCosEps)) continue;           // at or below the clamp: a value, no gradient
        const M3 h0 = {qg.n0.x / qg.l0, qg.n0.y / qg.l0, qg.n0.z / qg.l0}, h1 = {qg.n1.x / qg.l1, qg.n1.y / qg.l1, qg.n1.z / qg.l1};
        const float c = m_dot(h0, h1);
        // d(1 - cos) / d n0 and / d n1
        const M3 g0 = {-(h1.x - c * h0.x) / qg.l0, -(h1.y - c * h0.y) / qg.l0, -(h1.z - c * h0.z) / qg.l0};
        const M3 g1 = {-(h0.x - c * h1.x) / qg.l1, -(h0.y - c * h1.y) / qg.l1, -(h0.z - c * h1.z) / qg.l1};
        // n0 = e x p0: d / d p0 = g0 x e, d / d e = p0 x g0;  n1 = -(e x p1): the same with the sign turned
        const M3 ga = m_cross(g0, qg.e), gbn = m_cross(g1, qg.e);            // gb = -gbn
        const M3 e0 = m_cross(qg.p0, g0), e1 = m_cross(qg.p1, g1);
        const M3 ge = {e0.x - e1.x, e0.y - e1.y, e0.z - e1.z};
        M3 r;
        if (role == 0) r = {-ge.x - ga.x + gbn.x, -ge.y - ga.y + gbn.y, -ge.z - ga.z + gbn.z};
        else if (role == 1) r = ge;
        else if (role == 2) r = ga;
        else r = {-gbn.x, -gbn.y, -gbn.z};
        a.x += r.x; a.y += r.y; a.z += r.z;
      }
      g.x += c_nc * a.x; g.y += c_nc * a.y; g.z += c_nc * a.z;
    }
    gv[3 * k] = g.x; gv[3 * k + 1] = g.y; gv[3 * k + 2] = g.z;
  }
}

int mesh_reg_blocks(const MeshTopoDev& t) {
  const int n = t.V > t.Q ? t.V : t.Q;
  const int nb = (n + 255) / 256;
  return nb < 65535 ? nb : 65535;                   // the kernels stride over what one grid row does not cover
}

hipError_t launch_mesh_reg_fwd(const MeshTopoDev& t, const float* verts, int B, float lam_lap, float lam_nc, float* unit, float* partial,
                               float* out, hipStream_t st) {
  const int nb = mesh_reg_blocks(t);
  hipLaunchKernelGGL(mesh_reg_fwd_kernel, dim3(B, nb), dim3(256), 0, st, t, verts, lam_lap != 0.f ? 1 : 0, lam_nc != 0.f ? 1 : 0, unit, partial);
  hipLaunchKernelGGL(mesh_reg_finish_kernel, dim3(1), dim3(256), 0, st, t, partial, (long)B * nb, B, lam_lap, lam_nc, out);
  return hipGetLastError();
}

hipError_t launch_mesh_reg_bwd(const MeshTopoDev& t, const float* verts, const float* unit, const float* gout, int B, float lam_lap,
                               float lam_nc, float* gverts, hipStream_t st) {
  const int nb = (t.V + 255) / 256;
  hipLaunchKernelGGL(mesh_reg_bwd_kernel, dim3(B, nb < 65535 ? nb : 65535), dim3(256), 0, st, t, verts, unit, gout, B, lam_lap, lam_nc, gverts);
  return hipGetLastError();
}

}  // namespace hifihr
