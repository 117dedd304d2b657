// Differentiable soft silhouette of the predicted mesh at the output resolution, and the two losses that are functions of it
// (include/hifihr.h: hifihr_soft_sil_fwd / _bwd, hifihr_soft_sil_loss_fwd / _bwd).
//
// Semantics: PyTorch3D's rasterize_meshes(blur_radius > 0) followed by sigmoid_alpha_blend (SoftSilhouetteShader) [recalled, like the
// rest of that boundary: parity is unpinned].  Per image and output pixel (one sample at the pixel centre, the renderer's aa is ignored):
//   a face with NDC corners v0, v1, v2 PARTICIPATES iff its three vertices have Z > 0, |area| > 1e-8 and (inside || dist < blur_radius),
//   dist = the minimum over its three edges of the SQUARED distance from the centre to the segment (blur_radius is compared with the
//   squared distance, as in PyTorch3D), d = inside ? -dist : dist;
//   S = sum over the participating faces, in face-index order, of softplus(-d / sigma);   alpha = 1 - exp(-S)
// which is 1 - prod_f (1 - sigmoid(-d_f / sigma)) written in the log domain: d alpha / d d_f = -exp(-S) sigmoid(-d_f / sigma) / sigma has
// no division by (1 - p_f).  A pixel without a participating face is exactly 0.
// Two departures from PyTorch3D: there is no faces_per_pixel cap (equal whenever K >= the number of participating faces), and a face with
// a vertex at or behind the camera plane is left out (PyTorch3D projects such a vertex through the division).
// The gradient goes to the vertices only; participation, inside, the nearest edge and the clamp of t are piecewise constant choices.
//
// Forward: a vertex pass (NDC x, y and Z per vertex into the workspace), then one workgroup of 256 threads per 16 x 16 pixel tile and
// image.  Faces are taken 256 at a time: lane l tests face l's bounding box, grown by sqrt(blur_radius) plus a rounding allowance, against
// the tile's NDC rectangle (a lane later skips a listed face whose grown box misses its own pixel); the survivors are compacted IN FACE ORDER into an LDS list (ballot / popcount prefix: no counter raced by
// lanes, so a pixel's sum has the same order and the same bits on every call) and every lane walks the list for its own pixel (all lanes
// read the same LDS address: a broadcast).  The list holds kSoftList = one chunk's worth of faces and is walked once per chunk, so a
// tile under any number of faces is handled in as many passes as there are chunks: nothing is ever truncated.
// Backward: the same tiling and list; per listed face the six NDC gradient components are summed over the tile's 256 pixels on chip (wave
// shuffle reduction, then LDS across the four waves) and ONE float atomic per component goes to the NDC-gradient buffer of the workspace
// per (face corner, tile): 24 B per (face, tile), a few MB per step at B = 32 (cdna_hip_programming.md Guideline 12).  A last pass applies
// the projection's chain rule and overwrites gverts.
#include <hip/hip_runtime.h>

#include <cmath>

#include "hifihr_internal.h"
#include "render_math.h"

namespace hifihr {
namespace {

constexpr int kSoftThreads = 256;
constexpr int kSoftWaves = kSoftThreads / 64;
constexpr int kSoftTile = 16;          // pixels per tile edge: one pixel per thread
constexpr int kSoftList = 256;         // faces the LDS list holds = faces tested per pass (tests/soft_sil_cases.py restates it)
static_assert(kSoftTile * kSoftTile == kSoftThreads && kSoftList == kSoftThreads, "one pixel and one tested face per thread");

struct SoftFace {
  float x0, y0, x1, y1, x2, y2;
  float bx0, bx1, by0, by1;      // the bounding box grown as for the tile test: a centre outside it cannot participate
};
__device__ __forceinline__ bool in_box(const SoftFace& f, float px, float py) { return px >= f.bx0 && px <= f.bx1 && py >= f.by0 && py <= f.by1; }

__device__ __forceinline__ float soft_wsum(float x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
  return x;
}

// squared distance from p to the segment a-b; *t = the clamped parameter of the closest point
__device__ __forceinline__ float seg_dist2(float px, float py, float ax, float ay, float bx, float by, float* t) {
  const float ex = bx - ax, ey = by - ay;
  const float l2 = ex * ex + ey * ey;
  float u = ((px - ax) * ex + (py - ay) * ey) / l2;
  u = fminf(fmaxf(u, 0.f), 1.f);                       // a NaN (a zero-length edge: such a face has no area and never gets here) becomes 0
  const float qx = ax + u * ex - px, qy = ay + u * ey - py;
  *t = u;
  return qx * qx + qy * qy;
}

// One pixel centre against one face that passed the face-level tests.  true: the face participates; *d = the signed squared distance,
// *edge = the nearest edge (0: v0-v1, 1: v1-v2, 2: v2-v0; the first of equals), *t its clamped parameter.
__device__ __forceinline__ bool soft_sample(const SoftFace& f, float px, float py, float blur, float* d, int* edge, float* t) {
  const float area = edge_fn(f.x2, f.y2, f.x0, f.y0, f.x1, f.y1);
  const float e0 = edge_fn(px, py, f.x1, f.y1, f.x2, f.y2);
  const float e1 = edge_fn(px, py, f.x2, f.y2, f.x0, f.y0);
  const float e2 = edge_fn(px, py, f.x0, f.y0, f.x1, f.y1);
  // e_i / area > 0 for all three: the signs agree and none is zero
  const bool inside = area > 0.f ? (e0 > 0.f && e1 > 0.f && e2 > 0.f) : (e0 < 0.f && e1 < 0.f && e2 < 0.f);
  float t0, t1, t2;
  const float d0 = seg_dist2(px, py, f.x0, f.y0, f.x1, f.y1, &t0);
  const float d1 = seg_dist2(px, py, f.x1, f.y1, f.x2, f.y2, &t1);
  const float d2 = seg_dist2(px, py, f.x2, f.y2, f.x0, f.y0, &t2);
  float dist = d0, tt = t0;
  int e = 0;
  if (d1 < dist) { dist = d1; tt = t1; e = 1; }
  if (d2 < dist) { dist = d2; tt = t2; e = 2; }
  *d = inside ? -dist : dist;
  *edge = e;
  *t = tt;
  return inside || dist < blur;
}

__device__ __forceinline__ float softplus_f(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }
__device__ __forceinline__ float sigmoid_f(float x) {
  const float e = expf(-fabsf(x));
  return x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
}

// ---- vertex pass: (X, Y, Z) -> (NDC x, NDC y, Z, 0), the projection of oracle/render_oracle.py project_ndc ----
__global__ __launch_bounds__(kSoftThreads) void soft_sil_vertex_kernel(const float* __restrict__ verts, const float* __restrict__ cam, int V,
                                                                       long n, float4* __restrict__ vndc) {
  const long i = (long)blockIdx.x * kSoftThreads + threadIdx.x;
  if (i >= n) return;
  const int b = (int)(i / V);
  const float X = verts[i * 3], Y = verts[i * 3 + 1], Z = verts[i * 3 + 2];
  const float fx = cam[b * 4], fy = cam[b * 4 + 1], px = cam[b * 4 + 2], py = cam[b * 4 + 3];
  vndc[i] = make_float4((X * fx + Z * px) / Z, (Y * fy + Z * py) / Z, Z, 0.f);
}

// The tile's face list, shared by the forward and the backward: faces base .. base + 255 are tested, one per thread; the survivors land in
// sFace / sIdx in face order.  Returns their number (uniform over the workgroup).  Two barriers inside; the caller puts one more behind
// its walk before the next call overwrites the list.
struct TileRect { float xlo, xhi, ylo, yhi; };
__device__ __forceinline__ int soft_list_chunk(const RenderDev& r, const float4* __restrict__ vb, int base, const TileRect& tr, float grow0,
                                               SoftFace* sFace, int* sIdx, int* sWaveCnt) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int f = base + tid;
  bool keep = false;
  SoftFace sf = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (f < r.F) {
    const float4 a = vb[r.faces[f * 3]], b = vb[r.faces[f * 3 + 1]], c = vb[r.faces[f * 3 + 2]];
    const float area = edge_fn(c.x, c.y, a.x, a.y, b.x, b.y);
    const bool front = a.z > 0.f && b.z > 0.f && c.z > 0.f;
    const float xmin = fminf(a.x, fminf(b.x, c.x)), xmax = fmaxf(a.x, fmaxf(b.x, c.x));
    const float ymin = fminf(a.y, fminf(b.y, c.y)), ymax = fmaxf(a.y, fmaxf(b.y, c.y));
    // a participating centre lies inside the face or closer than sqrt(blur) to one of its edges: inside the box grown by sqrt(blur).
    // The allowance -- 1e-4 of the radius, 1e-5 of the coordinates' size: hundreds of ulp -- covers the rounding of the distances and
    // of this test, so the list is a superset of the faces soft_sample() accepts.  A NaN fails every comparison: not listed.
    const float grow = grow0 + 1e-5f * (1.f + fmaxf(fmaxf(fabsf(xmin), fabsf(xmax)), fmaxf(fabsf(ymin), fabsf(ymax))));
    sf = SoftFace{a.x, a.y, b.x, b.y, c.x, c.y, xmin - grow, xmax + grow, ymin - grow, ymax + grow};
    keep = front && fabsf(area) > kRasterEps && xmin - grow <= tr.xhi && xmax + grow >= tr.xlo && ymin - grow <= tr.yhi && ymax + grow >= tr.ylo;
  }
  const unsigned long long m = __ballot(keep);
  if (lane == 0) sWaveCnt[wave] = __popcll(m);
  __syncthreads();
  int pos = __popcll(m & ((1ull << lane) - 1ull)), cnt = 0;
#pragma unroll
  for (int w = 0; w < kSoftWaves; ++w) {
    if (w < wave) pos += sWaveCnt[w];
    cnt += sWaveCnt[w];
  }
  if (keep) { sFace[pos] = sf; sIdx[pos] = f; }
  __syncthreads();
  return cnt;
}

__device__ __forceinline__ TileRect tile_rect(int tx, int ty, int H) {
  const int x1 = min(tx * kSoftTile + kSoftTile - 1, H - 1), y1 = min(ty * kSoftTile + kSoftTile - 1, H - 1);
  // pixel xi samples NDC pix_to_ndc(H - 1 - xi): decreasing in xi
  return TileRect{pix_to_ndc(H - 1 - x1, H), pix_to_ndc(H - 1 - tx * kSoftTile, H), pix_to_ndc(H - 1 - y1, H), pix_to_ndc(H - 1 - ty * kSoftTile, H)};
}

__global__ __launch_bounds__(kSoftThreads) void soft_sil_fwd_kernel(RenderDev r, const float4* __restrict__ vndc, int tiles, float sigma,
                                                                    float blur, float grow0, float* __restrict__ alpha,
                                                                    float* __restrict__ neglog) {
  __shared__ SoftFace sFace[kSoftList];
  __shared__ int sIdx[kSoftList];
  __shared__ int sWaveCnt[kSoftWaves];
  const int tid = threadIdx.x;
  const int tile = blockIdx.x % (tiles * tiles), b = blockIdx.x / (tiles * tiles);
  const int tx = tile % tiles, ty = tile / tiles;
  const int xi = tx * kSoftTile + (tid & 15), yi = ty * kSoftTile + (tid >> 4);
  const float px = pix_to_ndc(r.H - 1 - xi, r.H), py = pix_to_ndc(r.H - 1 - yi, r.H);
  const TileRect tr = tile_rect(tx, ty, r.H);
  const float4* vb = vndc + (size_t)b * r.V;
  float S = 0.f;
  for (int base = 0; base < r.F; base += kSoftList) {
    const int cnt = soft_list_chunk(r, vb, base, tr, grow0, sFace, sIdx, sWaveCnt);
    for (int j = 0; j < cnt; ++j) {
      float d, t;
      int e;
      if (in_box(sFace[j], px, py) && soft_sample(sFace[j], px, py, blur, &d, &e, &t)) S += softplus_f(-d / sigma);
    }
    __syncthreads();
  }
  if (xi < r.H && yi < r.H) {
    const size_t o = ((size_t)b * r.H + yi) * r.H + xi;
    alpha[o] = -expm1f(-S);                                  // 1 - exp(-S), without the cancellation at small S
    neglog[o] = S;
  }
}

__global__ __launch_bounds__(kSoftThreads) void soft_sil_bwd_kernel(RenderDev r, const float4* __restrict__ vndc, int tiles, float sigma,
                                                                    float blur, float grow0, const float* __restrict__ neglog,
                                                                    const float* __restrict__ galpha, float* __restrict__ gndc) {
  __shared__ SoftFace sFace[kSoftList];
  __shared__ int sIdx[kSoftList];
  __shared__ int sWaveCnt[kSoftWaves];
  __shared__ int sLive[kSoftWaves];
  __shared__ float sRed[kSoftWaves][kSoftList][6];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tile = blockIdx.x % (tiles * tiles), b = blockIdx.x / (tiles * tiles);
  const int tx = tile % tiles, ty = tile / tiles;
  const int xi = tx * kSoftTile + (tid & 15), yi = ty * kSoftTile + (tid >> 4);
  const float px = pix_to_ndc(r.H - 1 - xi, r.H), py = pix_to_ndc(r.H - 1 - yi, r.H);
  // d loss / d d_f = galpha * -exp(-S) sigmoid(-d_f / sigma) / sigma: the pixel's share of it; 0 = the pixel is skipped
  float scale = 0.f;
  if (xi < r.H && yi < r.H) {
    const size_t o = ((size_t)b * r.H + yi) * r.H + xi;
    const float g = galpha[o], e = expf(-neglog[o]);
    if (g != 0.f && e != 0.f) scale = -(g * e) / sigma;
  }
  const unsigned long long live = __ballot(scale != 0.f);
  if (lane == 0) sLive[wave] = live != 0ull;
  __syncthreads();
  if ((sLive[0] | sLive[1] | sLive[2] | sLive[3]) == 0) return;          // no pixel of the tile carries a gradient (uniform)
  const TileRect tr = tile_rect(tx, ty, r.H);
  const float4* vb = vndc + (size_t)b * r.V;
  float* gb = gndc + (size_t)b * r.V * 2;
  for (int base = 0; base < r.F; base += kSoftList) {
    const int cnt = soft_list_chunk(r, vb, base, tr, grow0, sFace, sIdx, sWaveCnt);
    for (int j = 0; j < cnt; ++j) {
      const SoftFace f = sFace[j];
      float g[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};               // d loss / d (x0, y0, x1, y1, x2, y2)
      float d, t;
      int e;
      bool mine = false;
      if (scale != 0.f && in_box(f, px, py) && soft_sample(f, px, py, blur, &d, &e, &t)) {
        float gd = scale * sigmoid_f(-d / sigma);                // d loss / d d_f
        if (d < 0.f) gd = -gd;                                   // d = -dist inside
        // nearest edge a-b, closest point a + t (b - a), q = that point - p:  d dist / d a = 2 (1 - t) q, d dist / d b = 2 t q -- for an
        // interior t (q is perpendicular to the edge) and for a clamped one (t = 0: 2 q on a; t = 1: 2 q on b) alike
        const float ax = e == 0 ? f.x0 : (e == 1 ? f.x1 : f.x2), ay = e == 0 ? f.y0 : (e == 1 ? f.y1 : f.y2);
        const float bx = e == 0 ? f.x1 : (e == 1 ? f.x2 : f.x0), by = e == 0 ? f.y1 : (e == 1 ? f.y2 : f.y0);
        const float qx = ax + t * (bx - ax) - px, qy = ay + t * (by - ay) - py;
        const float wa = 2.f * (1.f - t) * gd, wb = 2.f * t * gd;
        const int ia = e * 2, ib = ((e + 1) % 3) * 2;
#pragma unroll
        for (int k = 0; k < 3; ++k) {                            // (no dynamic register indexing: the corner is selected by compare)
          const float sa = ia == 2 * k ? wa : 0.f, sb = ib == 2 * k ? wb : 0.f;
          g[2 * k] = (sa + sb) * qx;
          g[2 * k + 1] = (sa + sb) * qy;
        }
        mine = true;
      }
      if (__ballot(mine) != 0ull) {                              // uniform over the wave
#pragma unroll
        for (int k = 0; k < 6; ++k) g[k] = soft_wsum(g[k]);
      }
      if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) sRed[wave][j][k] = g[k];     // zeros where no lane of the wave had a share
      }
    }
    __syncthreads();
    if (tid < cnt) {
      const int f = sIdx[tid];
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        const float s = ((sRed[0][tid][k] + sRed[1][tid][k]) + sRed[2][tid][k]) + sRed[3][tid][k];
        if (s != 0.f) atomicAdd(gb + (size_t)r.faces[f * 3 + (k >> 1)] * 2 + (k & 1), s);
      }
    }
    __syncthreads();
  }
}

// xn = fx X / Z + px, yn = fy Y / Z + py:  gX = gxn fx / Z, gY = gyn fy / Z, gZ = -(gxn fx X + gyn fy Y) / Z^2.  Overwrites gverts; a
// vertex no participating face touched has a zero NDC gradient and gets 0.
__global__ __launch_bounds__(kSoftThreads) void soft_sil_proj_bwd_kernel(const float* __restrict__ verts, const float* __restrict__ cam, int V,
                                                                         long n, const float* __restrict__ gndc, float* __restrict__ gverts) {
  const long i = (long)blockIdx.x * kSoftThreads + threadIdx.x;
  if (i >= n) return;
  const float gx = gndc[i * 2], gy = gndc[i * 2 + 1];
  float gX = 0.f, gY = 0.f, gZ = 0.f;
  if (gx != 0.f || gy != 0.f) {
    const int b = (int)(i / V);
    const float X = verts[i * 3], Y = verts[i * 3 + 1], Z = verts[i * 3 + 2];
    const float ax = gx * cam[b * 4] / Z, ay = gy * cam[b * 4 + 1] / Z;
    gX = ax;
    gY = ay;
    gZ = -(ax * X + ay * Y) / Z;
  }
  gverts[i * 3] = gX; gverts[i * 3 + 1] = gY; gverts[i * 3 + 2] = gZ;
}

// ---- losses: per image, in a fixed order, (sum |A - M|, sum A M, sum (A + M)) in fp64; no atomics ----
__device__ __forceinline__ float mask_at(const void* mask, int is_i64, size_t i) {
  return is_i64 ? (float)reinterpret_cast<const long long*>(mask)[i] : reinterpret_cast<const float*>(mask)[i];
}

__global__ __launch_bounds__(kSoftThreads) void soft_sil_loss_sums_kernel(const float* __restrict__ alpha, const void* __restrict__ mask,
                                                                          int is_i64, int HW, double* __restrict__ sums) {
  __shared__ double red[kSoftWaves][3];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double s[3] = {0.0, 0.0, 0.0};
  for (int i = tid; i < HW; i += kSoftThreads) {
    const size_t o = (size_t)b * HW + i;
    const float a = alpha[o], m = mask_at(mask, is_i64, o);
    s[0] += (double)fabsf(a - m);
    s[1] += (double)a * (double)m;
    s[2] += (double)a + (double)m;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s[k] += __shfl_down(s[k], o, 64);
    if (lane == 0) red[wave][k] = s[k];
  }
  __syncthreads();
  if (tid < 3) sums[(size_t)b * 3 + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// out = (lam_s mean |A - M|, lam_i (1 - mean_b I_b / U_b)), U_b = sum (A + M) - I_b: losses.iou, no epsilon -- an image with U_b = 0
// gives NaN.  A term whose weight is exactly 0 is written as 0, whatever its value would be.
__global__ void soft_sil_loss_finish_kernel(const double* __restrict__ sums, int B, int HW, float lam_s, float lam_i, float* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double l1 = 0.0, ratio = 0.0;
  for (int b = 0; b < B; ++b) {
    l1 += sums[b * 3];
    ratio += sums[b * 3 + 1] / (sums[b * 3 + 2] - sums[b * 3 + 1]);
  }
  out[0] = lam_s == 0.f ? 0.f : (float)((double)lam_s * (l1 / ((double)B * (double)HW)));
  out[1] = lam_i == 0.f ? 0.f : (float)((double)lam_i * (1.0 - ratio / (double)B));
}

// gA = gout[0] lam_s sign(A - M) / (B HW) - gout[1] lam_i / B * (M U - I (1 - M)) / U^2        (d U / d A = 1 - M)
__global__ __launch_bounds__(kSoftThreads) void soft_sil_loss_bwd_kernel(const float* __restrict__ alpha, const void* __restrict__ mask,
                                                                         int is_i64, const double* __restrict__ sums,
                                                                         const float* __restrict__ gout, int B, int HW, float lam_s,
                                                                         float lam_i, float* __restrict__ galpha) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * kSoftThreads + threadIdx.x;
  if (i >= HW) return;
  const size_t o = (size_t)b * HW + i;
  const float a = alpha[o], m = mask_at(mask, is_i64, o);
  float g = 0.f;
  if (lam_s != 0.f) {
    const float sg = a > m ? 1.f : (a < m ? -1.f : 0.f);
    g = gout[0] * lam_s * sg / ((float)B * (float)HW);
  }
  if (lam_i != 0.f) {
    const double I = sums[b * 3 + 1], U = sums[b * 3 + 2] - I;
    g -= gout[1] * lam_i / (float)B * (float)(((double)m * U - I * (1.0 - (double)m)) / (U * U));
  }
  galpha[o] = g;
}

// workspace: float4 vndc[B][V], then float gndc[B][V][2]
inline float* gndc_of(const RenderDev& r, int B, void* ws) { return reinterpret_cast<float*>(reinterpret_cast<float4*>(ws) + (size_t)B * r.V); }
inline float grow_of(float blur) { return sqrtf(blur) * 1.0001f; }
inline bool grid_ok(const RenderDev& r, int B, int* tiles) {
  *tiles = (r.H + kSoftTile - 1) / kSoftTile;
  return (long long)B * *tiles * *tiles <= 0x7fffffffLL && ((long long)B * r.V + kSoftThreads - 1) / kSoftThreads <= 0x7fffffffLL;
}

}  // namespace

size_t soft_sil_workspace_bytes(const RenderDev& r, int B) { return (size_t)B * r.V * (sizeof(float4) + 2 * sizeof(float)); }

hipError_t launch_soft_sil_fwd(const RenderDev& r, const float* verts, const float* cam, int B, float sigma, float blur, float* alpha,
                               float* neglog, void* ws, hipStream_t st) {
  int tiles;
  if (B <= 0 || !grid_ok(r, B, &tiles)) return hipErrorInvalidValue;
  const long n = (long)B * r.V;
  float4* vndc = reinterpret_cast<float4*>(ws);
  hipLaunchKernelGGL(soft_sil_vertex_kernel, dim3((unsigned)((n + kSoftThreads - 1) / kSoftThreads)), dim3(kSoftThreads), 0, st, verts, cam, r.V, n, vndc);
  hipLaunchKernelGGL(soft_sil_fwd_kernel, dim3((unsigned)(B * tiles * tiles)), dim3(kSoftThreads), 0, st, r, vndc, tiles, sigma, blur,
                     grow_of(blur), alpha, neglog);
  return hipGetLastError();
}

hipError_t launch_soft_sil_bwd(const RenderDev& r, const float* verts, const float* cam, const float* neglog, const float* galpha, int B,
                               float sigma, float blur, float* gverts, void* ws, hipStream_t st) {
  int tiles;
  if (B <= 0 || !grid_ok(r, B, &tiles)) return hipErrorInvalidValue;
  const long n = (long)B * r.V;
  float4* vndc = reinterpret_cast<float4*>(ws);
  float* gndc = gndc_of(r, B, ws);
  const dim3 vgrid((unsigned)((n + kSoftThreads - 1) / kSoftThreads));
  hipError_t e = hipMemsetAsync(gndc, 0, sizeof(float) * 2 * (size_t)n, st);      // the tiles of an image add into it
  if (e != hipSuccess) return e;
  // the vertex pass again: the backward depends on nothing the forward left in the workspace
  hipLaunchKernelGGL(soft_sil_vertex_kernel, vgrid, dim3(kSoftThreads), 0, st, verts, cam, r.V, n, vndc);
  hipLaunchKernelGGL(soft_sil_bwd_kernel, dim3((unsigned)(B * tiles * tiles)), dim3(kSoftThreads), 0, st, r, vndc, tiles, sigma, blur,
                     grow_of(blur), neglog, galpha, gndc);
  hipLaunchKernelGGL(soft_sil_proj_bwd_kernel, vgrid, dim3(kSoftThreads), 0, st, verts, cam, r.V, n, gndc, gverts);
  return hipGetLastError();
}

hipError_t launch_soft_sil_loss_fwd(const float* alpha, const void* mask, int mask_i64, int B, int HW, float lam_s, float lam_i, double* sums,
                                    float* out, hipStream_t st) {
  if (B <= 0 || HW <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(soft_sil_loss_sums_kernel, dim3((unsigned)B), dim3(kSoftThreads), 0, st, alpha, mask, mask_i64, HW, sums);
  hipLaunchKernelGGL(soft_sil_loss_finish_kernel, dim3(1), dim3(64), 0, st, sums, B, HW, lam_s, lam_i, out);
  return hipGetLastError();
}

hipError_t launch_soft_sil_loss_bwd(const float* alpha, const void* mask, int mask_i64, const double* sums, const float* gout, int B, int HW,
                                    float lam_s, float lam_i, float* galpha, hipStream_t st) {
  if (B <= 0 || HW <= 0 || B > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(soft_sil_loss_bwd_kernel, dim3((unsigned)((HW + kSoftThreads - 1) / kSoftThreads), (unsigned)B), dim3(kSoftThreads), 0, st,
                     alpha, mask, mask_i64, sums, gout, B, HW, lam_s, lam_i, galpha);
  return hipGetLastError();
}

}  // namespace hifihr
