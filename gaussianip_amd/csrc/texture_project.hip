// texture_project.hip — rendered views projected onto the UV texture of a triangle mesh: every owned texel of the atlas of
// gaussianip_amd/utils/texture.py gathers its colour from the K images that see its point of the surface, weighted by the viewing
// angle (DESIGN.md "Baking a texture from rendered views").  Linked into libgip_model.so.
//
// Definition, everything in float32 in the operand order written here (the library is built with -ffp-contract=off: no product is
// fused into a sum).  Face f lives in cell q = f / 2 (row q / n, column q % n, n = T / cell cells per row) as half h = f & 1; a texel
// with cell-local indices (i, j) belongs to half (i + j >= cell) and is owned when its cell's row and column are < n and its face
// id is < F.  With (li, lj) = (i, j) for half 0 and (cell - 1 - i, cell - 1 - j) for half 1, b = cell - 3, e1 = v1 - v0, e2 = v2 - v0
// (vertices in WORLD coordinates):
//     p  = (v0 + (li / b) e1) + (lj / b) e2                      per component, true divisions
//     n  = e1 x e2 = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x),   nn = (nx nx + ny ny) + nz nz
// A face with nn == 0 (or NaN) contributes nothing.  For the views k = 0 .. K - 1 in that order, view k being M (16 values, row-vector
// convention: clip = (p, 1) M), the camera centre cam (3) and a pad in view[k * 20 ..]:
//   1  clip_j = ((px M[0][j] + py M[1][j]) + pz M[2][j]) + M[3][j] for j = x, y, w;  skip unless w > 0
//   2  sx = ((clip_x / w) * 0.5 + 0.5) * W,  sy = ((clip_y / w) * 0.5 + 0.5) * H  (mr_snap's mapping: pixel (ix, iy) has its centre at
//      (ix + 0.5, iy + 0.5));  skip unless 0 <= sx < W and 0 <= sy < H
//   3  ix = floor(sx), iy = floor(sy), wp = vis_depth[k, iy, ix];  skip unless wp > 0;  skip if w - wp > depth_tolerance (occluded)
//   4  d = cam - p,  dd = (dx dx + dy dy) + dz dz,  cos = ((nx dx + ny dy) + nz dz) / (sqrt(nn) * sqrt(dd)),  |cos| when two_sided;
//      skip unless cos >= min_cos
//   5  bilinear lookup of images[k] ([H, W, 4] interleaved r, g, b, a) at (x, y) = (sx - 0.5, sy - 0.5): xf = floor(x), fx = x - xf,
//      columns clamp(xf, 0, W - 1) and clamp(xf + 1, 0, W - 1), rows likewise (mr_bilinear's rule), each channel
//      (1 - fy) ((1 - fx) t00 + fx t01) + fy ((1 - fx) t10 + fx t11);  skip unless a >= min_alpha;  unpremultiply: rgb = rgb / a
//   6  wt = cos * cos;  weight_sum += wt;  color_sum += wt * rgb (per channel);  count += 1
// Owned texels are written (zeros and a count of 0 when no view passes); unowned texels are never written.  No atomics: a texel
// belongs to one lane, so two runs are bitwise equal.
//
//   texture_project_kernel  grid = (T / 16, T / 16) rounded up, 256 lanes: a 16 x 16 block of texels, each wavefront an 8 x 8
//                           square of it, so that with cells of side 8 or more a wavefront's lanes lie in at most four cells (eight
//                           consecutive faces, which the extractor emits close in space) and project to neighbouring pixels of a view.
//                           The view table is staged in LDS once per workgroup and read from there at a wave-uniform address
//                           (a broadcast).  Owner and (li, lj) are integer arithmetic in registers; there is no point array.  A
//                           lane of an unowned texel leaves after the barrier.  Every bilinear tap is one 16-byte load.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gip_model.h"

#define TP_THREADS 256
#define TP_TILE 16                              // the workgroup's block of texels is TP_TILE x TP_TILE
#define TP_MAX_VIEWS 64
#define TP_VIEW 20                              // floats of a view: full_proj_transform (16), camera centre (3), pad
#define TP_MAX_SIZE 16384                       // texture side, as gip_texture_bake's
#define TP_MAX_IMAGE 16384                      // image side, as the mesh rasterizer's

__global__ void __launch_bounds__(TP_THREADS)
texture_project_kernel(const float* __restrict__ vertices, int V, const int32_t* __restrict__ faces, int F, int T, int cell, int K,
                       const float* __restrict__ view, const float4* __restrict__ images, const float* __restrict__ vis_depth, int H,
                       int W, float depth_tolerance, float min_cos, float min_alpha, int two_sided, int unpremultiply,
                       float* __restrict__ color_sum, float* __restrict__ weight_sum, int32_t* __restrict__ count) {
  __shared__ float s_view[TP_MAX_VIEWS * TP_VIEW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < K * TP_VIEW; i += TP_THREADS) s_view[i] = view[i];
  __syncthreads();
  const int x = (int)blockIdx.x * TP_TILE + (wave & 1) * 8 + (lane & 7), y = (int)blockIdx.y * TP_TILE + (wave >> 1) * 8 + (lane >> 3);
  if (x >= T || y >= T) return;
  const int n = T / cell, col = x / cell, row = y / cell;
  if (col >= n || row >= n) return;
  const int i = x - col * cell, j = y - row * cell, h = (i + j >= cell) ? 1 : 0;
  const int f = 2 * (row * n + col) + h;   // < 2 n^2 <= 2 (T / 4)^2 < 2^31
  if (f >= F) return;
  const int li = h ? cell - 1 - i : i, lj = h ? cell - 1 - j : j;
  // indices clipped so that no face, whatever the caller wrote there, leads outside the vertices
  const int i0 = min(max(faces[(int64_t)f * 3], 0), V - 1), i1 = min(max(faces[(int64_t)f * 3 + 1], 0), V - 1),
            i2 = min(max(faces[(int64_t)f * 3 + 2], 0), V - 1);
  const float* v0 = vertices + (int64_t)i0 * 3;
  const float* v1 = vertices + (int64_t)i1 * 3;
  const float* v2 = vertices + (int64_t)i2 * 3;
  const float fleg = (float)(cell - 3);
  const float a = (float)li / fleg, b = (float)lj / fleg;
  const float e1x = v1[0] - v0[0], e1y = v1[1] - v0[1], e1z = v1[2] - v0[2];
  const float e2x = v2[0] - v0[0], e2y = v2[1] - v0[1], e2z = v2[2] - v0[2];
  const float px = (v0[0] + a * e1x) + b * e2x, py = (v0[1] + a * e1y) + b * e2y, pz = (v0[2] + a * e1z) + b * e2z;
  const float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
  const float nn = (nx * nx + ny * ny) + nz * nz;
  float cr = 0.f, cg = 0.f, cb = 0.f, ws = 0.f;
  int cnt = 0;
  if (nn > 0.f) {
    const float nlen = sqrtf(nn);
    const float fW = (float)W, fH = (float)H;
    for (int k = 0; k < K; k++) {
      const float* m = s_view + k * TP_VIEW;
      const float w = ((px * m[3] + py * m[7]) + pz * m[11]) + m[15];
      if (!(w > 0.f)) continue;
      const float cx = ((px * m[0] + py * m[4]) + pz * m[8]) + m[12];
      const float cy = ((px * m[1] + py * m[5]) + pz * m[9]) + m[13];
      const float sx = ((cx / w) * 0.5f + 0.5f) * fW, sy = ((cy / w) * 0.5f + 0.5f) * fH;
      if (!(sx >= 0.f && sx < fW && sy >= 0.f && sy < fH)) continue;
      const int ix = (int)floorf(sx), iy = (int)floorf(sy);   // 0 .. W - 1, 0 .. H - 1 by the test above
      const int64_t base = (int64_t)k * H * W;
      const float wp = vis_depth[base + (int64_t)iy * W + ix];
      if (!(wp > 0.f) || w - wp > depth_tolerance) continue;
      const float dx = m[16] - px, dy = m[17] - py, dz = m[18] - pz;
      const float dd = (dx * dx + dy * dy) + dz * dz;
      float c = ((nx * dx + ny * dy) + nz * dz) / (nlen * sqrtf(dd));
      if (two_sided) c = fabsf(c);
      if (!(c >= min_cos)) continue;
      const float bx = sx - 0.5f, by = sy - 0.5f;
      const float xf = floorf(bx), yf = floorf(by);   // -1 .. W - 1, -1 .. H - 1
      const float fx = bx - xf, fy = by - yf;
      const int xi = (int)xf, yi = (int)yf;
      const int x0 = min(max(xi, 0), W - 1), x1 = min(max(xi + 1, 0), W - 1), y0 = min(max(yi, 0), H - 1), y1 = min(max(yi + 1, 0), H - 1);
      const float4 t00 = images[base + (int64_t)y0 * W + x0], t01 = images[base + (int64_t)y0 * W + x1],
                   t10 = images[base + (int64_t)y1 * W + x0], t11 = images[base + (int64_t)y1 * W + x1];
      const float gx = 1.f - fx, gy = 1.f - fy;
      const float al = gy * (gx * t00.w + fx * t01.w) + fy * (gx * t10.w + fx * t11.w);
      if (!(al >= min_alpha)) continue;
      float r = gy * (gx * t00.x + fx * t01.x) + fy * (gx * t10.x + fx * t11.x);
      float g = gy * (gx * t00.y + fx * t01.y) + fy * (gx * t10.y + fx * t11.y);
      float bl = gy * (gx * t00.z + fx * t01.z) + fy * (gx * t10.z + fx * t11.z);
      if (unpremultiply) {
        r = r / al;
        g = g / al;
        bl = bl / al;
      }
      const float wt = c * c;
      ws += wt;
      cr += wt * r;
      cg += wt * g;
      cb += wt * bl;
      cnt++;
    }
  }
  const int64_t o = (int64_t)y * T + x;
  color_sum[o * 3] = cr;
  color_sum[o * 3 + 1] = cg;
  color_sum[o * 3 + 2] = cb;
  weight_sum[o] = ws;
  count[o] = cnt;
}

extern "C" int gip_texture_project(const float* vertices, int64_t V, const int32_t* faces, int64_t F, int32_t T, int32_t cell, int32_t K,
                                   const float* views, const float* images, const float* vis_depth, int32_t H, int32_t W,
                                   float depth_tolerance, float min_cos, float min_alpha, int32_t two_sided, int32_t unpremultiply,
                                   float* color_sum, float* weight_sum, int32_t* count, void* stream) {
  if (K < 1 || K > TP_MAX_VIEWS) return 1;
  if (F < 0 || F > INT32_MAX || V < 0 || V > INT32_MAX) return 1;
  if (T < 4 || T > TP_MAX_SIZE || cell < 4 || cell > T) return 1;
  const int64_t n = T / cell;
  if (2 * n * n < F) return 1;
  if (H < 1 || W < 1 || H > TP_MAX_IMAGE || W > TP_MAX_IMAGE) return 1;
  if (unpremultiply && !(min_alpha > 0.f)) return 1;   // a division by an alpha of 0
  if (F == 0) return 0;
  if (!vertices || V == 0 || !faces || !views || !images || !vis_depth || !color_sum || !weight_sum || !count) return 1;
  if (((uintptr_t)images & 15) != 0) return 1;   // a tap is one 16-byte load
  const unsigned tiles = (unsigned)((T + TP_TILE - 1) / TP_TILE);
  hipLaunchKernelGGL(texture_project_kernel, dim3(tiles, tiles), dim3(TP_THREADS), 0, (hipStream_t)stream, vertices, (int)V, faces, (int)F,
                     (int)T, (int)cell, (int)K, views, (const float4*)images, vis_depth, (int)H, (int)W, depth_tolerance, min_cos, min_alpha,
                     (int)two_sided, (int)unpremultiply, color_sum, weight_sum, count);
  return hipGetLastError() == hipSuccess ? 0 : 3;
}
