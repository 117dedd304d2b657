// Differentiable depth map of the hard render, and the masked depth loss (include/hifihr.h "Depth map": hifihr_render_depth_fwd / _bwd,
// hifihr_depth_loss_fwd / _bwd).
//
// The rasteriser (csrc/render.hip) finds every sample's nearest face and its perspective-correct depth pz, keeps face_id and drops pz.
// The forward here is one pass over that face_id: one lane per OUTPUT pixel re-evaluates its aa x aa samples through sample_face() of
// render_math.h -- the routine the rasteriser and oracle/raster_oracle.c decide coverage with, so at aa = 1 the depth has the bits of the
// rasteriser's own zbuf -- and averages the covered ones (the background never enters the average).  A run of samples on one face
// projects the face once.
// Backward (the atomic form): one wave per tile of 8 x 8 output pixels, a lane per pixel with its aa^2 face indices in registers.  A pass
// first names up to 64 of the tile's distinct faces with cross-lane moves alone (no memory access in that serial part), then lane n
// projects face n -- one round of loads for all of them -- into an LDS record; every lane sums the gradient of its samples into the
// nine LDS sums of their faces (NDC x, y and Z of the three corners; a run of samples on one face is merged in registers first), and
// lane n issues ONE float atomic per component and corner of face n into the per-vertex accumulator float[B][V][3] of the workspace:
// 9 atomics per (face, tile) instead of 9 per covered sample (MI355X_MICROARCH.md "Global float atomics").  A tile under more than 64
// faces takes further passes.  A per-vertex pass applies the projection's chain rule and overwrites gverts.  The sums on chip and
// over tiles are in atomic order: gverts is reproducible to rounding, not bitwise, as for hifihr_render_bwd.
// (First form: the wave took one face per round -- project it, a nine-fold shuffle reduction, nine atomics.  Each round waited for its own
// loads: 0.69 ms at B = 32 on the MANO topology, 4.7 x hifihr_render_bwd; profiles/depth_time.txt holds the form kept.)
#include <hip/hip_runtime.h>

#include <cmath>

#include "hifihr_internal.h"
#include "render_math.h"

namespace hifihr {
namespace {

constexpr int kDepthThreads = 256;
constexpr int kDepthWaves = kDepthThreads / 64;
constexpr int kDepthTile = 8;          // output pixels per tile edge of the backward: one wave per tile, one pixel per lane
static_assert(kDepthTile * kDepthTile == 64, "one pixel per lane of a wave");

struct DepthFace {
  FaceXYZ f;
  float xmin, xmax, ymin, ymax;
};

// face fid of image b: the projection of render_vertex_kernel (csrc/render.hip), expression for expression, and the bounding box of
// stage_b2.  fid is inside 0 .. F - 1 (the callers check it); the renderer checked faces[] against V when it was created.
__device__ __forceinline__ DepthFace depth_face(const RenderDev& r, const float* __restrict__ vb, float fx, float fy, float px, float py, int fid) {
  float x[3], y[3], z[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int v = r.faces[3 * fid + k];
    const float X = vb[3 * v], Y = vb[3 * v + 1], Z = vb[3 * v + 2];
    x[k] = (X * fx + Z * px) / Z;
    y[k] = (Y * fy + Z * py) / Z;
    z[k] = Z;
  }
  DepthFace d;
  d.f.x0 = x[0]; d.f.y0 = y[0]; d.f.x1 = x[1]; d.f.y1 = y[1]; d.f.x2 = x[2]; d.f.y2 = y[2]; d.f.z0 = z[0]; d.f.z1 = z[1]; d.f.z2 = z[2];
  d.xmin = fminf(x[0], fminf(x[1], x[2])); d.xmax = fmaxf(x[0], fmaxf(x[1], x[2]));
  d.ymin = fminf(y[0], fminf(y[1], y[2])); d.ymax = fmaxf(y[0], fmaxf(y[1], y[2]));
  return d;
}

template <int AA>
__global__ __launch_bounds__(kDepthThreads) void render_depth_fwd_kernel(RenderDev r, const float* __restrict__ verts, const float* __restrict__ cam,
                                                                         const int* __restrict__ face_id, long n, float* __restrict__ depth,
                                                                         int* __restrict__ hits) {
  const long i = (long)blockIdx.x * kDepthThreads + threadIdx.x;
  if (i >= n) return;
  const int H = r.H, S = H * AA;
  const int xi = (int)(i % H), yi = (int)((i / H) % H), b = (int)(i / ((long)H * H));
  const float fx = cam[4 * b], fy = cam[4 * b + 1], px = cam[4 * b + 2], py = cam[4 * b + 3];
  const float* vb = verts + (size_t)b * r.V * 3;
  const int* fb = face_id + (size_t)b * S * S;
  float sum = 0.f;
  int cnt = 0, last = -1;
  DepthFace d;
#pragma unroll
  for (int si = 0; si < AA; ++si) {
    const int sy = yi * AA + si;
    const float ys = pix_to_ndc(S - 1 - sy, S);
#pragma unroll
    for (int sj = 0; sj < AA; ++sj) {
      const int sx = xi * AA + sj;
      const int fid = fb[(size_t)sy * S + sx];
      if (fid < 0 || fid >= r.F) continue;
      if (fid != last) { d = depth_face(r, vb, fx, fy, px, py, fid); last = fid; }
      float bary[3], pz;
      if (sample_face(d.f, d.xmin, d.xmax, d.ymin, d.ymax, pix_to_ndc(S - 1 - sx, S), ys, bary, &pz)) { sum += pz; ++cnt; }
    }
  }
  depth[i] = cnt > 0 ? sum / (float)cnt : 0.f;
  hits[i] = cnt;
}

constexpr int kDepthFaces = 64;        // distinct faces a tile handles per pass: one per lane (a tile under more faces takes more passes)

template <int AA>
__global__ __launch_bounds__(64) void render_depth_bwd_kernel(RenderDev r, const float* __restrict__ verts, const float* __restrict__ cam,
                                                              const int* __restrict__ face_id, const float* __restrict__ gdepth,
                                                              const int* __restrict__ hits, int tiles, float* __restrict__ gacc) {
  __shared__ FaceXYZ sFace[kDepthFaces];                       // the pass's faces, projected once each
  __shared__ float sAcc[kDepthFaces][9];                       // their gradient summed over the tile: (NDC x, NDC y, Z) of the three corners
  const int lane = threadIdx.x;
  const int tile = blockIdx.x % (tiles * tiles), b = blockIdx.x / (tiles * tiles);
  const int xi = (tile % tiles) * kDepthTile + (lane & 7), yi = (tile / tiles) * kDepthTile + (lane >> 3);
  const int H = r.H, S = H * AA;
  int fid[AA * AA], slot[AA * AA];
#pragma unroll
  for (int k = 0; k < AA * AA; ++k) fid[k] = -1;
  float gs = 0.f;                                              // the share of a covered sample: gdepth / hits
  if (xi < H && yi < H) {
    const size_t o = ((size_t)b * H + yi) * H + xi;
    const int h = hits[o];
    const float g = gdepth[o];
    if (h > 0 && g != 0.f) {
      gs = g / (float)h;
      const int* fb = face_id + (size_t)b * S * S;
#pragma unroll
      for (int k = 0; k < AA * AA; ++k) {
        const int f = fb[(size_t)(yi * AA + k / AA) * S + xi * AA + k % AA];
        fid[k] = (f >= 0 && f < r.F) ? f : -1;
      }
    }
  }
  const float fx = cam[4 * b], fy = cam[4 * b + 1], px = cam[4 * b + 2], py = cam[4 * b + 3];
  const float* vb = verts + (size_t)b * r.V * 3;
  float* gb = gacc + (size_t)b * r.V * 3;
  for (;;) {
    // name up to 64 of the tile's distinct pending faces, registers and cross-lane moves only: the first pending sample of the first lane
    // that has one names the next face, every lane marks its samples on it.  Lane n keeps face n.
    int n = 0, myf = -1;
#pragma unroll
    for (int k = 0; k < AA * AA; ++k) slot[k] = -1;
    while (n < kDepthFaces) {
      int mine = -1;
#pragma unroll
      for (int k = AA * AA - 1; k >= 0; --k) mine = (fid[k] >= 0 && slot[k] < 0) ? fid[k] : mine;
      const unsigned long long m = __ballot(mine >= 0);
      if (m == 0ull) break;                                    // uniform; every round names one more face
      const int f = __shfl(mine, __builtin_ctzll(m), 64);
#pragma unroll
      for (int k = 0; k < AA * AA; ++k) slot[k] = fid[k] == f ? n : slot[k];
      if (lane == n) myf = f;
      ++n;
    }
    if (n == 0) break;                                         // uniform: nothing pending
    if (lane < n) sFace[lane] = depth_face(r, vb, fx, fy, px, py, myf).f;      // all the pass's faces at once: one round of loads
#pragma unroll
    for (int c = 0; c < 9; ++c) sAcc[lane][c] = 0.f;
    __syncthreads();
    // every lane adds its samples' gradients into their faces' LDS sums; a run of samples on one face is summed in registers first
    int cur = -1;
    float g[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < AA * AA; ++k) {
      if (slot[k] >= 0) {
        if (slot[k] != cur) {
          if (cur >= 0) {
#pragma unroll
            for (int c = 0; c < 9; ++c) atomicAdd(&sAcc[cur][c], g[c]);
          }
          cur = slot[k];
#pragma unroll
          for (int c = 0; c < 9; ++c) g[c] = 0.f;
        }
        float t[9];
        pz_bwd(sFace[cur], pix_to_ndc(S - 1 - (xi * AA + k % AA), S), pix_to_ndc(S - 1 - (yi * AA + k / AA), S), gs, t);
#pragma unroll
        for (int c = 0; c < 9; ++c) g[c] += t[c];
        fid[k] = -1;                                           // done
      }
    }
    if (cur >= 0) {
#pragma unroll
      for (int c = 0; c < 9; ++c) atomicAdd(&sAcc[cur][c], g[c]);
    }
    __syncthreads();
    if (lane < n) {                                            // one float atomic per component, corner and (face, tile)
#pragma unroll
      for (int c = 0; c < 9; ++c) {
        const float v = sAcc[lane][c];
        if (v != 0.f) atomicAdd(gb + (size_t)r.faces[3 * myf + c / 3] * 3 + c % 3, v);
      }
    }
    __syncthreads();                                           // the next pass overwrites the LDS records
  }
}

// xn = fx X / Z + px, yn = fy Y / Z + py, and Z itself:  gX = gxn fx / Z, gY = gyn fy / Z, gZ = gz - (gX X + gY Y) / Z.  Overwrites gverts;
// a vertex no covered sample references has a zero accumulator and gets exactly 0.
__global__ __launch_bounds__(kDepthThreads) void render_depth_proj_bwd_kernel(const float* __restrict__ verts, const float* __restrict__ cam, int V,
                                                                              long n, const float* __restrict__ gacc, float* __restrict__ gverts) {
  const long i = (long)blockIdx.x * kDepthThreads + threadIdx.x;
  if (i >= n) return;
  const float gx = gacc[i * 3], gy = gacc[i * 3 + 1], gz = gacc[i * 3 + 2];
  float gX = 0.f, gY = 0.f, gZ = 0.f;
  if (gx != 0.f || gy != 0.f || gz != 0.f) {
    const int b = (int)(i / V);
    const float X = verts[i * 3], Y = verts[i * 3 + 1], Z = verts[i * 3 + 2];
    gX = gx * cam[b * 4] / Z;
    gY = gy * cam[b * 4 + 1] / Z;
    gZ = gz - (gX * X + gY * Y) / Z;
  }
  gverts[i * 3] = gX; gverts[i * 3 + 1] = gY; gverts[i * 3 + 2] = gZ;
}

// ---- loss: per image, in a fixed order and in fp64, (sum over valid pixels of |d - D|, their count); no atomics ----
__device__ __forceinline__ bool depth_mask_set(const void* mask, int is_i64, size_t i) {
  if (mask == nullptr) return true;
  return is_i64 ? reinterpret_cast<const long long*>(mask)[i] != 0 : reinterpret_cast<const float*>(mask)[i] != 0.f;
}
// valid: hits > 0, D > 0, M != 0 and (trunc == 0 or |d - D| <= trunc); *diff = d - D in fp64 (exact)
__device__ __forceinline__ bool depth_valid(const float* __restrict__ depth, const int* __restrict__ hits, const float* __restrict__ target,
                                            const void* __restrict__ mask, int is_i64, size_t o, float trunc, double* diff) {
  const float D = target[o];
  if (hits[o] <= 0 || !(D > 0.f) || !depth_mask_set(mask, is_i64, o)) return false;
  const double e = (double)depth[o] - (double)D;
  if (trunc != 0.f && !(fabs(e) <= (double)trunc)) return false;
  *diff = e;
  return true;
}

__global__ __launch_bounds__(kDepthThreads) void depth_loss_sums_kernel(const float* __restrict__ depth, const int* __restrict__ hits,
                                                                        const float* __restrict__ target, const void* __restrict__ mask, int is_i64,
                                                                        int HW, float trunc, double* __restrict__ sums) {
  __shared__ double red[kDepthWaves][2];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double s[2] = {0.0, 0.0};
  for (int i = tid; i < HW; i += kDepthThreads) {
    double e;
    if (depth_valid(depth, hits, target, mask, is_i64, (size_t)b * HW + i, trunc, &e)) { s[0] += fabs(e); s[1] += 1.0; }
  }
#pragma unroll
  for (int k = 0; k < 2; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s[k] += __shfl_down(s[k], o, 64);
    if (lane == 0) red[wave][k] = s[k];
  }
  __syncthreads();
  if (tid < 2) sums[(size_t)b * 2 + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// out = lam sum_b sum_b / max(sum_b count_b, 1): a batch without a valid pixel gives exactly 0
__global__ void depth_loss_finish_kernel(const double* __restrict__ sums, int B, float lam, float* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double s = 0.0, n = 0.0;
  for (int b = 0; b < B; ++b) { s += sums[b * 2]; n += sums[b * 2 + 1]; }
  out[0] = (float)((double)lam * (s / fmax(n, 1.0)));
}

// gdepth = gout lam sign(d - D) / max(count, 1) on the valid pixels, 0 elsewhere (and where d == D)
__global__ __launch_bounds__(kDepthThreads) void depth_loss_bwd_kernel(const float* __restrict__ depth, const int* __restrict__ hits,
                                                                       const float* __restrict__ target, const void* __restrict__ mask, int is_i64,
                                                                       const double* __restrict__ sums, const float* __restrict__ gout, int B, int HW,
                                                                       float lam, float trunc, float* __restrict__ gdepth) {
  __shared__ float sScale;
  if (threadIdx.x == 0) {
    double n = 0.0;
    for (int b = 0; b < B; ++b) n += sums[b * 2 + 1];
    sScale = (float)((double)gout[0] * (double)lam / fmax(n, 1.0));
  }
  __syncthreads();
  const int b = blockIdx.y;
  const int i = blockIdx.x * kDepthThreads + threadIdx.x;
  if (i >= HW) return;
  const size_t o = (size_t)b * HW + i;
  double e;
  float g = 0.f;
  if (depth_valid(depth, hits, target, mask, is_i64, o, trunc, &e)) g = e > 0.0 ? sScale : (e < 0.0 ? -sScale : 0.f);
  gdepth[o] = g;
}

inline bool depth_grid_ok(const RenderDev& r, int B, int* tiles) {
  *tiles = (r.H + kDepthTile - 1) / kDepthTile;
  const long long px = (long long)B * r.H * r.H, vt = (long long)B * r.V;
  return (long long)B * *tiles * *tiles <= 0x7fffffffLL && (px + kDepthThreads - 1) / kDepthThreads <= 0x7fffffffLL &&
         (vt + kDepthThreads - 1) / kDepthThreads <= 0x7fffffffLL;
}

}  // namespace

// workspace of the backward: the per-vertex accumulator float gacc[B][V][3] = d loss / d (NDC x, NDC y, Z)
size_t render_depth_workspace_bytes(const RenderDev& r, int B) { return ((size_t)B * r.V * 3 * sizeof(float) + 15) / 16 * 16; }

hipError_t launch_render_depth_fwd(const RenderDev& r, const float* verts, const float* cam, const int* face_id, int B, float* depth, int* hits,
                                   hipStream_t st) {
  int tiles;
  if (B <= 0 || !depth_grid_ok(r, B, &tiles)) return hipErrorInvalidValue;
  const long n = (long)B * r.H * r.H;
  const dim3 grid((unsigned)((n + kDepthThreads - 1) / kDepthThreads)), block(kDepthThreads);
  switch (r.aa) {
    case 1: hipLaunchKernelGGL(render_depth_fwd_kernel<1>, grid, block, 0, st, r, verts, cam, face_id, n, depth, hits); break;
    case 2: hipLaunchKernelGGL(render_depth_fwd_kernel<2>, grid, block, 0, st, r, verts, cam, face_id, n, depth, hits); break;
    case 3: hipLaunchKernelGGL(render_depth_fwd_kernel<3>, grid, block, 0, st, r, verts, cam, face_id, n, depth, hits); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_render_depth_bwd(const RenderDev& r, const float* verts, const float* cam, const int* face_id, const float* gdepth,
                                   const int* hits, int B, float* gverts, void* ws, hipStream_t st) {
  int tiles;
  if (B <= 0 || !depth_grid_ok(r, B, &tiles) || r.aa < 1 || r.aa > 3) return hipErrorInvalidValue;
  const long n = (long)B * r.V;
  float* gacc = reinterpret_cast<float*>(ws);
  hipError_t e = hipMemsetAsync(gacc, 0, sizeof(float) * 3 * (size_t)n, st);      // the tiles of an image add into it
  if (e != hipSuccess) return e;
  const dim3 grid((unsigned)(B * tiles * tiles)), block(64);
  switch (r.aa) {
    case 1: hipLaunchKernelGGL(render_depth_bwd_kernel<1>, grid, block, 0, st, r, verts, cam, face_id, gdepth, hits, tiles, gacc); break;
    case 2: hipLaunchKernelGGL(render_depth_bwd_kernel<2>, grid, block, 0, st, r, verts, cam, face_id, gdepth, hits, tiles, gacc); break;
    default: hipLaunchKernelGGL(render_depth_bwd_kernel<3>, grid, block, 0, st, r, verts, cam, face_id, gdepth, hits, tiles, gacc); break;
  }
  hipLaunchKernelGGL(render_depth_proj_bwd_kernel, dim3((unsigned)((n + kDepthThreads - 1) / kDepthThreads)), dim3(kDepthThreads), 0, st, verts, cam,
                     r.V, n, gacc, gverts);
  return hipGetLastError();
}

hipError_t launch_depth_loss_fwd(const float* depth, const int* hits, const float* target, const void* mask, int mask_i64, int B, int HW, float lam,
                                 float trunc, double* sums, float* out, hipStream_t st) {
  if (B <= 0 || HW <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(depth_loss_sums_kernel, dim3((unsigned)B), dim3(kDepthThreads), 0, st, depth, hits, target, mask, mask_i64, HW, trunc, sums);
  hipLaunchKernelGGL(depth_loss_finish_kernel, dim3(1), dim3(64), 0, st, sums, B, lam, out);
  return hipGetLastError();
}

hipError_t launch_depth_loss_bwd(const float* depth, const int* hits, const float* target, const void* mask, int mask_i64, const double* sums,
                                 const float* gout, int B, int HW, float lam, float trunc, float* gdepth, hipStream_t st) {
  if (B <= 0 || HW <= 0 || B > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(depth_loss_bwd_kernel, dim3((unsigned)((HW + kDepthThreads - 1) / kDepthThreads), (unsigned)B), dim3(kDepthThreads), 0, st,
                     depth, hits, target, mask, mask_i64, sums, gout, B, HW, lam, trunc, gdepth);
  return hipGetLastError();
}

}  // namespace hifihr
