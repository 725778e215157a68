// mesh_raster.hip — a triangle rasterizer for the exported textured mesh: coverage and visibility, perspective-correct attribute
// interpolation, a bilinear texture lookup with its gradients, and the fused shade of gaussianip_amd.utils.rasterize.render_mesh
// (DESIGN.md "Rendering the mesh").  Linked into libgip_model.so, compiled with its -ffp-contract=off.
//
// Definition of coverage and visibility (tests/mesh_render_reference.py restates it; the forward is bit-reproducible).
//   * Input is clip-space positions pos [B, V, 4] float32 and tri [F, 3] int32, one topology for all B views.
//   * The pixel (px, py) has its centre at NDC ((2 px + 1) / W - 1, (2 py + 1) / H - 1).  Row index grows with NDC y.  This is the
//     Gaussian rasterizer's ndc2Pix, so verts_h @ camera.full_proj_transform lands pixel for pixel on the Gaussian render.
//   * Per vertex, in float32, in this operand order: ndc = x / w; s = (ndc * 0.5f + 0.5f) * W; X = (int) rintf(s * 256.0f), which
//     gives 8 sub-pixel bits.  The same holds for Y with H.  The division is correctly rounded.
//   * A triangle is dropped whole in any of three cases: a vertex has w <= 0 (or a NaN w); a snapped coordinate exceeds +-2^22 in
//     magnitude (the guard band; a NaN counts as exceeding it); its integer area (X1 - X0)(Y2 - Y0) - (Y1 - Y0)(X2 - X0) is zero.
//     There is no polygon clipping.  A triangle with a vertex index outside [0, V) is dropped as well.
//   * Coverage uses exact integer edge functions in int64 at the pixel centre P = (256 px + 128, 256 py + 128), normalised by the
//     sign of the area:  E0 = (X2 - X1)(Py - Y1) - (Y2 - Y1)(Px - X1),  E1 = (X0 - X2)(Py - Y2) - (Y0 - Y2)(Px - X2),
//     E2 = (X1 - X0)(Py - Y0) - (Y1 - Y0)(Px - X0), all three and the area negated when the area is negative.  Both windings are
//     drawn; cull_backfaces drops negative area.  A pixel is covered when every E_i > 0, or E_i == 0 on an edge that owns its
//     points: the top-left fill rule, here in the form "the edge's direction (dx, dy) = sign(area) (end - start) has dy < 0, or
//     dy == 0 and dx > 0" (the sample point moved by an infinitesimal (+1, +0)), so a shared edge or vertex has exactly one owner.
//   * Screen-space weights b_i = (float) E_i / (float) area.  Depth d = b0 * (z0 / w0) + b1 * (z1 / w1) + b2 * (z2 / w2), float32,
//     left to right.  Fragments with d < -1 or d > 1 (or a NaN d) are discarded; -0 counts as +0.
//   * Visibility: a fragment's key is the order-preserving 32-bit image of d (bits ^ 0x80000000 for d >= 0, ~bits for d < 0),
//     shifted left by 32 bits and OR-ed with the triangle index.  The smallest 64-bit key wins: the nearest fragment, and at equal
//     depth the lower triangle index; a 64-bit unsigned atomic minimum on a [B, H, W] key buffer, so the result does not depend on
//     the order of execution.
//   * rast [B, H, W, 4] = (u, v, d, triangle index + 1), all zeros at an empty pixel; u, v are the perspective-correct weights of
//     corners 0 and 1: q_i = b_i / w_i, u = q0 / ((q0 + q1) + q2), v = q1 / ((q0 + q1) + q2).
//   * Interpolation: a = (u * a0 + v * a1) + ((1 - u) - v) * a2.  Lookup at uv = (s, t), (0, 0) the corner of tex[0, 0], texel
//     centres at (i + 0.5) / T: x = s * Tw - 0.5, x0 = floor(x), fx = x - x0, the indices x0, x0 + 1 clamped to the border, the same
//     in y;  value = (1 - fy) * ((1 - fx) * t00 + fx * t01) + fy * ((1 - fx) * t10 + fx * t11).
//
//   mesh_setup_kernel           one lane per (view, triangle): snaps the three vertices, classifies, walks the bounding box of a small
//                               triangle (at most MR_SMALL_MAX pixel centres) with incrementally updated edge functions, appends a
//                               larger one to a list (a wavefront's larger ones take their slots with one atomic add).
//   mesh_large_kernel           one wavefront per listed triangle, lanes striding over the bounding box.
//   mesh_resolve_kernel         one lane per pixel: key -> rast, one 16-byte store.
//   mesh_shade_kernel           one lane per pixel: face-varying uv [F, 3, 2] interpolated (flip_v: every corner's v replaced by 1 - v
//                               first, the OBJ convention), texture [Th, Tw, 3] looked up, (r, g, b, alpha) over the background in one
//                               16-byte store.
//   mesh_shade_backward_kernel  dL/dcolor scattered to the four texels with float atomic adds (and to the corners' uv when asked
//                               for): not bit-reproducible.  No gradient reaches vertex positions.
//   mesh_interpolate_kernel / mesh_interpolate_backward_kernel / mesh_texture_kernel / mesh_texture_backward_kernel: the unfused
//                               pieces with any channel count.
// The triangle set-up (mr_load), the perspective weights (mr_persp), the lookup with its gradients (mr_tap*) and the fused shade's set-up
// (mr_shade) live in mesh_raster_common.h, which mesh_grad.hip (gradients to positions, antialias) and mesh_mip.hip (mipmaps) share.
#include "mesh_raster_common.h"

#define MR_SMALL_MAX 64        // pixel centres in the bounding box up to which the setup lane rasterizes the triangle itself (tuning)
#define MR_LARGE_BLOCKS 1024   // workgroups of the cooperative kernel (4 wavefronts each, striding over the list)

typedef unsigned long long mr_key;

// the smallest value of E that still counts as inside: 0 on an edge that owns its points, 1 on the others
__device__ __forceinline__ int mr_bias(int dx, int dy) { return (dy < 0 || (dy == 0 && dx > 0)) ? 0 : 1; }

__device__ __forceinline__ void mr_biases(const MrTri& t, int& c0, int& c1, int& c2) {
  c0 = mr_bias(t.sgn * (t.X2 - t.X1), t.sgn * (t.Y2 - t.Y1));
  c1 = mr_bias(t.sgn * (t.X0 - t.X2), t.sgn * (t.Y0 - t.Y2));
  c2 = mr_bias(t.sgn * (t.X1 - t.X0), t.sgn * (t.Y1 - t.Y0));
}

__device__ __forceinline__ void mr_fragment(const MrTri& t, int64_t e0, int64_t e1, int64_t e2, uint32_t f, mr_key* __restrict__ at) {
  float b0, b1, b2;
  mr_weights(t, e0, e1, e2, b0, b1, b2);
  const float d = b0 * t.zw0 + b1 * t.zw1 + b2 * t.zw2;
  if (!(d >= -1.f && d <= 1.f)) return;
  atomicMin(at, ((mr_key)mesh_float_key(d) << 32) | f);
}

// the pixel centres inside the bounding box, clipped to the image; false when there is none
__device__ __forceinline__ bool mr_box(const MrTri& t, int H, int W, int& x_lo, int& x_hi, int& y_lo, int& y_hi) {
  const int minX = min(t.X0, min(t.X1, t.X2)), maxX = max(t.X0, max(t.X1, t.X2));
  const int minY = min(t.Y0, min(t.Y1, t.Y2)), maxY = max(t.Y0, max(t.Y1, t.Y2));
  x_lo = max((minX + 127) >> 8, 0);      // the first px with 256 px + 128 >= minX
  x_hi = min((maxX - 128) >> 8, W - 1);  // the last px with 256 px + 128 <= maxX
  y_lo = max((minY + 127) >> 8, 0);
  y_hi = min((maxY - 128) >> 8, H - 1);
  return x_lo <= x_hi && y_lo <= y_hi;
}

// ------------------------------------------------------------------------------------------------------------------ setup
__global__ void __launch_bounds__(MR_THREADS)
mesh_setup_kernel(const float* __restrict__ pos, const int32_t* __restrict__ tri, int B, int V, int F, int H, int W, int cull,
                  mr_key* __restrict__ keys, uint32_t* __restrict__ large_count, int32_t* __restrict__ large_list) {
  const int64_t g = (int64_t)blockIdx.x * MR_THREADS + threadIdx.x;
  const bool live = g < (int64_t)B * F;
  const int b = live ? (int)(g / F) : 0, f = live ? (int)(g - (int64_t)b * F) : 0;
  MrTri t;
  int x_lo = 0, x_hi = -1, y_lo = 0, y_hi = -1;
  int kind = 0;   // 0: nothing to draw, 1: rasterized here, 2: listed
  if (live && mr_load(pos + (int64_t)b * V * 4, tri, f, V, H, W, cull, t) && mr_box(t, H, W, x_lo, x_hi, y_lo, y_hi))
    kind = (int64_t)(x_hi - x_lo + 1) * (y_hi - y_lo + 1) > MR_SMALL_MAX ? 2 : 1;
  // the wavefront's listed triangles take their slots with one add; every (view, triangle) is appended at most once: the list holds B * F
  const unsigned long long big = __ballot(kind == 2);
  if (big) {
    const int lane = threadIdx.x & 63, leader = __ffsll((long long)big) - 1;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(large_count, (uint32_t)__popcll(big));
    base = (uint32_t)__shfl((int)base, leader);
    if (kind == 2) large_list[base + (uint32_t)__popcll(big & ((1ull << lane) - 1ull))] = (int32_t)g;
  }
  if (kind != 1) return;
  int c0, c1, c2;
  mr_biases(t, c0, c1, c2);
  int64_t r0, r1, r2;
  mr_edges(t, 256 * x_lo + 128, 256 * y_lo + 128, r0, r1, r2);
  int64_t sx0, sy0, sx1, sy1, sx2, sy2;
  mr_steps(t, sx0, sy0, sx1, sy1, sx2, sy2);
  mr_key* view = keys + (int64_t)b * H * W;
  for (int py = y_lo; py <= y_hi; py++) {
    int64_t e0 = r0, e1 = r1, e2 = r2;
    for (int px = x_lo; px <= x_hi; px++) {
      if (e0 >= c0 && e1 >= c1 && e2 >= c2) mr_fragment(t, e0, e1, e2, (uint32_t)f, view + (int64_t)py * W + px);
      e0 += sx0;
      e1 += sx1;
      e2 += sx2;
    }
    r0 += sy0;
    r1 += sy1;
    r2 += sy2;
  }
}

// ------------------------------------------------------------------------------------------------------------------ large triangles
__global__ void __launch_bounds__(MR_THREADS)
mesh_large_kernel(const float* __restrict__ pos, const int32_t* __restrict__ tri, int B, int V, int F, int H, int W, int cull,
                  mr_key* __restrict__ keys, const uint32_t* __restrict__ large_count, const int32_t* __restrict__ large_list) {
  const int lane = threadIdx.x & 63;
  const int64_t total = (int64_t)B * F;
  const int64_t count = min((int64_t)large_count[0], total);
  for (int64_t i = (int64_t)blockIdx.x * (MR_THREADS / 64) + (threadIdx.x >> 6); i < count; i += (int64_t)gridDim.x * (MR_THREADS / 64)) {
    const int64_t g = large_list[i];
    if (g < 0 || g >= total) continue;
    const int b = (int)(g / F), f = (int)(g - (int64_t)b * F);
    MrTri t;
    int x_lo, x_hi, y_lo, y_hi;
    if (!mr_load(pos + (int64_t)b * V * 4, tri, f, V, H, W, cull, t) || !mr_box(t, H, W, x_lo, x_hi, y_lo, y_hi)) continue;
    int c0, c1, c2;
    mr_biases(t, c0, c1, c2);
    const int bw = x_hi - x_lo + 1;
    const int n = bw * (y_hi - y_lo + 1);   // <= H * W < 2^31
    mr_key* view = keys + (int64_t)b * H * W;
    for (int k = lane; k < n; k += 64) {
      const int row = k / bw, px = x_lo + (k - row * bw), py = y_lo + row;
      int64_t e0, e1, e2;
      mr_edges(t, 256 * px + 128, 256 * py + 128, e0, e1, e2);
      if (e0 >= c0 && e1 >= c1 && e2 >= c2) mr_fragment(t, e0, e1, e2, (uint32_t)f, view + (int64_t)py * W + px);
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------ resolve
__global__ void __launch_bounds__(MR_THREADS)
mesh_resolve_kernel(const float* __restrict__ pos, const int32_t* __restrict__ tri, int B, int V, int F, int H, int W,
                    const mr_key* __restrict__ keys, float4* __restrict__ rast) {
  const int64_t g = (int64_t)blockIdx.x * MR_THREADS + threadIdx.x;
  if (g >= (int64_t)B * H * W) return;
  const mr_key key = keys[g];
  float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
  const uint32_t f = (uint32_t)key;
  if (key != ~0ull && f < (uint32_t)F) {
    const MrPixel p = mr_pixel(g, H, W);
    MrTri t;
    if (mr_load(pos + (int64_t)p.b * V * 4, tri, (int)f, V, H, W, 0, t)) {
      const float d = mesh_key_float((uint32_t)(key >> 32));
      const MrPersp w = mr_persp(t, p.px, p.py);
      out = make_float4(w.q0 / w.S, w.q1 / w.S, d, (float)(f + 1));
    }
  }
  rast[g] = out;
}

// ------------------------------------------------------------------------------------------------------------------ fused shade
__global__ void __launch_bounds__(MR_THREADS)
mesh_shade_kernel(const float4* __restrict__ rast, const float* __restrict__ uv, const float* __restrict__ tex, const float* __restrict__ bg,
                  int64_t pixels, int F, int flip_v, int Th, int Tw, float4* __restrict__ shaded) {
  const int64_t g = (int64_t)blockIdx.x * MR_THREADS + threadIdx.x;
  if (g >= pixels) return;
  const float4 r = rast[g];
  const int f = (int)r.w - 1;
  float4 out = make_float4(bg[0], bg[1], bg[2], 0.f);
  if (f >= 0 && f < F) {
    const MrShade h = mr_shade(r, uv, f, flip_v);
    const MrTap q = mr_tap(h.s, h.t, Th, Tw, 3, 0);
    out = make_float4(mr_tap_mix(q, tex, 0), mr_tap_mix(q, tex, 1), mr_tap_mix(q, tex, 2), 1.f);
  }
  shaded[g] = out;
}

__global__ void __launch_bounds__(MR_THREADS)
mesh_shade_backward_kernel(const float4* __restrict__ rast, const float* __restrict__ uv, const float* __restrict__ tex,
                           const float4* __restrict__ g_shaded, int64_t pixels, int F, int flip_v, int Th, int Tw, float* __restrict__ g_tex,
                           float* __restrict__ g_uv) {
  const int64_t g = (int64_t)blockIdx.x * MR_THREADS + threadIdx.x;
  if (g >= pixels) return;
  const float4 r = rast[g];
  const int f = (int)r.w - 1;
  if (f < 0 || f >= F) return;
  const float4 go = g_shaded[g];
  const float gc[3] = {go.x, go.y, go.z};
  const MrShade h = mr_shade(r, uv, f, flip_v);
  const MrTap q = mr_tap(h.s, h.t, Th, Tw, 3, 0);
  float gs = 0.f, gt = 0.f;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    if (g_tex) mr_tap_scatter(q, g_tex, c, gc[c]);
    if (g_uv) mr_tap_slopes(q, tex, c, gc[c], gs, gt);
  }
  if (g_uv) {
    gs *= (float)Tw;
    gt *= flip_v ? -(float)Th : (float)Th;   // d(1 - v) / dv
    float* o = g_uv + (int64_t)f * 6;
    atomicAdd(o + 0, r.x * gs);
    atomicAdd(o + 1, r.x * gt);
    atomicAdd(o + 2, r.y * gs);
    atomicAdd(o + 3, r.y * gt);
    atomicAdd(o + 4, h.w * gs);
    atomicAdd(o + 5, h.w * gt);
  }
}

// ------------------------------------------------------------------------------------------------------------------ the unfused pieces
__global__ void __launch_bounds__(MR_THREADS)
mesh_interpolate_kernel(const float* __restrict__ attr, int64_t attr_stride, const int32_t* __restrict__ idx, const float4* __restrict__ rast,
                        int64_t pixels, int64_t per_view, int F, int N, int C, float* __restrict__ out) {
  const int64_t g = (int64_t)blockIdx.x * MR_THREADS + threadIdx.x;
  if (g >= pixels) return;
  const float4 r = rast[g];
  float* o = out + g * C;
  int64_t i0, i1, i2;
  if (!mr_corners(r, idx, F, N, i0, i1, i2)) {
    for (int c = 0; c < C; c++) o[c] = 0.f;
    return;
  }
  const float* a = attr + (g / per_view) * attr_stride;
  const float w = (1.f - r.x) - r.y;
  for (int c = 0; c < C; c++) o[c] = mr_interp(r.x, r.y, w, a[i0 * C + c], a[i1 * C + c], a[i2 * C + c]);
}

__global__ void __launch_bounds__(MR_THREADS)
mesh_interpolate_backward_kernel(const float* __restrict__ g_out, const int32_t* __restrict__ idx, const float4* __restrict__ rast,
                                 int64_t pixels, int64_t per_view, int F, int N, int C, float* __restrict__ g_attr, int64_t attr_stride) {
  const int64_t g = (int64_t)blockIdx.x * MR_THREADS + threadIdx.x;
  if (g >= pixels) return;
  const float4 r = rast[g];
  int64_t i0, i1, i2;
  if (!mr_corners(r, idx, F, N, i0, i1, i2)) return;
  float* a = g_attr + (g / per_view) * attr_stride;
  const float* go = g_out + g * C;
  const float w = (1.f - r.x) - r.y;
  for (int c = 0; c < C; c++) {
    const float v = go[c];
    atomicAdd(a + i0 * C + c, r.x * v);
    atomicAdd(a + i1 * C + c, r.y * v);
    atomicAdd(a + i2 * C + c, w * v);
  }
}

__global__ void __launch_bounds__(MR_THREADS)
mesh_texture_kernel(const float* __restrict__ tex, int64_t tex_stride, const float2* __restrict__ uv, int64_t pixels, int64_t per_view, int Th,
                    int Tw, int C, float* __restrict__ out) {
  const int64_t g = (int64_t)blockIdx.x * MR_THREADS + threadIdx.x;
  if (g >= pixels) return;
  const float2 st = uv[g];
  const MrTap q = mr_tap(st.x, st.y, Th, Tw, C, (g / per_view) * tex_stride);
  float* o = out + g * C;
  for (int c = 0; c < C; c++) o[c] = mr_tap_mix(q, tex, c);
}

__global__ void __launch_bounds__(MR_THREADS)
mesh_texture_backward_kernel(const float* __restrict__ tex, int64_t tex_stride, const float2* __restrict__ uv, const float* __restrict__ g_out,
                             int64_t pixels, int64_t per_view, int Th, int Tw, int C, float* __restrict__ g_tex, float2* __restrict__ g_uv) {
  const int64_t g = (int64_t)blockIdx.x * MR_THREADS + threadIdx.x;
  if (g >= pixels) return;
  const float2 st = uv[g];
  const MrTap q = mr_tap(st.x, st.y, Th, Tw, C, (g / per_view) * tex_stride);
  const float* go = g_out + g * C;
  float gs = 0.f, gt = 0.f;
  for (int c = 0; c < C; c++) {
    const float v = go[c];
    if (g_tex) mr_tap_scatter(q, g_tex, c, v);
    if (g_uv) mr_tap_slopes(q, tex, c, v, gs, gt);
  }
  if (g_uv) g_uv[g] = make_float2(gs * (float)Tw, gt * (float)Th);
}

// ------------------------------------------------------------------------------------------------------------------ C-ABI
extern "C" int gip_mesh_raster_workspace_size(int32_t B, int32_t H, int32_t W, int64_t F, size_t* bytes) {
  if (!bytes || !mr_image_ok(B, H, W) || F < 0 || F > MR_MAX_FACES || (int64_t)B * F > INT32_MAX) return 1;
  // keys [B, H, W] of 8 bytes, the list's count (16 bytes, keeping the list aligned), the list [B * F] int32
  *bytes = (size_t)B * H * W * sizeof(mr_key) + 16 + (size_t)B * F * sizeof(int32_t);
  return 0;
}

extern "C" int gip_mesh_rasterize(const float* pos, const int32_t* tri, int32_t B, int64_t V, int64_t F, int32_t H, int32_t W,
                                  int32_t cull_backfaces, void* workspace, size_t workspace_bytes, float* rast, void* stream) {
  size_t need = 0;
  if (gip_mesh_raster_workspace_size(B, H, W, F, &need) != 0) return 1;
  if (V < 0 || V > INT32_MAX || !rast) return 1;
  hipStream_t st = (hipStream_t)stream;
  const int64_t pixels = (int64_t)B * H * W;
  if (F == 0 || V == 0) return hipMemsetAsync(rast, 0, (size_t)pixels * 16, st) == hipSuccess ? 0 : 3;
  if (!pos || !tri || !workspace || workspace_bytes < need) return 1;
  mr_key* keys = (mr_key*)workspace;
  uint32_t* count = (uint32_t*)(keys + pixels);
  int32_t* list = (int32_t*)(count + 4);
  if (hipMemsetAsync(keys, 0xFF, (size_t)pixels * sizeof(mr_key), st) != hipSuccess) return 3;
  if (hipMemsetAsync(count, 0, 16, st) != hipSuccess) return 3;
  hipLaunchKernelGGL(mesh_setup_kernel, dim3(mesh_blocks((int64_t)B * F)), dim3(MR_THREADS), 0, st, pos, tri, (int)B, (int)V, (int)F, (int)H,
                     (int)W, (int)(cull_backfaces != 0), keys, count, list);
  const int64_t waves = (int64_t)B * F;
  const unsigned large = (unsigned)((waves + 3) / 4 < MR_LARGE_BLOCKS ? (waves + 3) / 4 : MR_LARGE_BLOCKS);
  hipLaunchKernelGGL(mesh_large_kernel, dim3(large), dim3(MR_THREADS), 0, st, pos, tri, (int)B, (int)V, (int)F, (int)H, (int)W,
                     (int)(cull_backfaces != 0), keys, (const uint32_t*)count, (const int32_t*)list);
  hipLaunchKernelGGL(mesh_resolve_kernel, dim3(mesh_blocks(pixels)), dim3(MR_THREADS), 0, st, pos, tri, (int)B, (int)V, (int)F, (int)H, (int)W,
                     (const mr_key*)keys, (float4*)rast);
  return mesh_done();
}

extern "C" int gip_mesh_interpolate(const float* attr, int32_t attr_batch, int64_t N, int32_t C, const int32_t* idx, int64_t F,
                                    const float* rast, int32_t B, int32_t H, int32_t W, float* out, void* stream) {
  if (!mr_attr_ok(attr, attr_batch, N, C, idx, F, B, H, W) || !rast || !out) return 1;
  const int64_t pixels = (int64_t)B * H * W;
  hipLaunchKernelGGL(mesh_interpolate_kernel, dim3(mesh_blocks(pixels)), dim3(MR_THREADS), 0, (hipStream_t)stream, attr,
                     mr_stride(attr_batch, N * C), idx, (const float4*)rast, pixels, (int64_t)H * W, (int)F, (int)N, (int)C, out);
  return mesh_done();
}

extern "C" int gip_mesh_interpolate_backward(const float* g_out, int32_t attr_batch, int64_t N, int32_t C, const int32_t* idx, int64_t F,
                                             const float* rast, int32_t B, int32_t H, int32_t W, float* g_attr, void* stream) {
  if (!mr_attr_ok(g_attr, attr_batch, N, C, idx, F, B, H, W) || !rast || !g_out) return 1;
  if (N == 0) return 0;
  if (!g_attr) return 1;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(g_attr, 0, (size_t)attr_batch * N * C * sizeof(float), st) != hipSuccess) return 3;
  const int64_t pixels = (int64_t)B * H * W;
  hipLaunchKernelGGL(mesh_interpolate_backward_kernel, dim3(mesh_blocks(pixels)), dim3(MR_THREADS), 0, st, g_out, idx, (const float4*)rast,
                     pixels, (int64_t)H * W, (int)F, (int)N, (int)C, g_attr, mr_stride(attr_batch, N * C));
  return mesh_done();
}

extern "C" int gip_mesh_texture(const float* tex, int32_t tex_batch, int32_t Th, int32_t Tw, int32_t C, const float* uv, int32_t B,
                                int32_t H, int32_t W, float* out, void* stream) {
  if (!mr_batch_ok(B, H, W, tex_batch) || !mr_tex_ok(Th, Tw, C) || !tex || !uv || !out) return 1;
  const int64_t pixels = (int64_t)B * H * W;
  hipLaunchKernelGGL(mesh_texture_kernel, dim3(mesh_blocks(pixels)), dim3(MR_THREADS), 0, (hipStream_t)stream, tex,
                     mr_stride(tex_batch, (int64_t)Th * Tw * C), (const float2*)uv, pixels, (int64_t)H * W, (int)Th, (int)Tw, (int)C,
                     out);
  return mesh_done();
}

extern "C" int gip_mesh_texture_backward(const float* tex, int32_t tex_batch, int32_t Th, int32_t Tw, int32_t C, const float* uv,
                                         const float* g_out, int32_t B, int32_t H, int32_t W, float* g_tex, float* g_uv, void* stream) {
  if (!mr_batch_ok(B, H, W, tex_batch) || !mr_tex_ok(Th, Tw, C) || !tex || !uv || !g_out) return 1;
  if (!g_tex && !g_uv) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (g_tex && hipMemsetAsync(g_tex, 0, (size_t)tex_batch * Th * Tw * C * sizeof(float), st) != hipSuccess) return 3;
  const int64_t pixels = (int64_t)B * H * W;
  hipLaunchKernelGGL(mesh_texture_backward_kernel, dim3(mesh_blocks(pixels)), dim3(MR_THREADS), 0, st, tex,
                     mr_stride(tex_batch, (int64_t)Th * Tw * C), (const float2*)uv, g_out, pixels, (int64_t)H * W, (int)Th, (int)Tw,
                     (int)C, g_tex, (float2*)g_uv);
  return mesh_done();
}

extern "C" int gip_mesh_shade(const float* rast, const float* uv, int64_t F, int32_t flip_v, const float* tex, int32_t Th, int32_t Tw, const float* bg,
                              int32_t B, int32_t H, int32_t W, float* shaded, void* stream) {
  if (!mr_image_ok(B, H, W) || !mr_tex_ok(Th, Tw, 3) || F < 0 || F > MR_MAX_FACES || !rast || !tex || !bg || !shaded) return 1;
  if (F > 0 && !uv) return 1;
  const int64_t pixels = (int64_t)B * H * W;
  hipLaunchKernelGGL(mesh_shade_kernel, dim3(mesh_blocks(pixels)), dim3(MR_THREADS), 0, (hipStream_t)stream, (const float4*)rast, uv, tex, bg,
                     pixels, (int)F, (int)(flip_v != 0), (int)Th, (int)Tw, (float4*)shaded);
  return mesh_done();
}

extern "C" int gip_mesh_shade_backward(const float* rast, const float* uv, int64_t F, int32_t flip_v, const float* tex, int32_t Th, int32_t Tw,
                                       const float* g_shaded, int32_t B, int32_t H, int32_t W, float* g_tex, float* g_uv, void* stream) {
  if (!mr_image_ok(B, H, W) || !mr_tex_ok(Th, Tw, 3) || F < 0 || F > MR_MAX_FACES || !rast || !tex || !g_shaded) return 1;
  if (F > 0 && !uv) return 1;
  if (!g_tex && !g_uv) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (g_tex && hipMemsetAsync(g_tex, 0, (size_t)Th * Tw * 3 * sizeof(float), st) != hipSuccess) return 3;
  if (g_uv && F > 0 && hipMemsetAsync(g_uv, 0, (size_t)F * 6 * sizeof(float), st) != hipSuccess) return 3;
  if (F == 0) return 0;
  const int64_t pixels = (int64_t)B * H * W;
  hipLaunchKernelGGL(mesh_shade_backward_kernel, dim3(mesh_blocks(pixels)), dim3(MR_THREADS), 0, st, (const float4*)rast, uv, tex,
                     (const float4*)g_shaded, pixels, (int)F, (int)(flip_v != 0), (int)Th, (int)Tw, g_tex, g_uv);
  return mesh_done();
}
