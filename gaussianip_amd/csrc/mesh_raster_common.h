// mesh_raster_common.h — what mesh_raster.hip (the forward, the attribute and texture gradients), mesh_grad.hip (the gradients to
// positions, the antialias pass) and mesh_mip.hip (differentials, mipmaps) share: a triangle as the definition of mesh_raster.hip's header
// sees it, a pixel's perspective weights, the attribute rows a pixel's triangle names, the bilinear lookup with its gradients, the fused
// shade's set-up, and the entry points' shape checks.  All three are compiled with -ffp-contract=off; every device function here is inlined.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gip_model.h"
#include "mesh_common.h"      // the depth test's float key; mesh_blocks (the *_ok checks below keep every count inside INT32_MAX), mesh_done

#define MR_THREADS MESH_THREADS
#define MR_GUARD 4194304.f     // 2^22: the guard band of snapped coordinates
#define MR_MAX_SIZE 16384      // image side: 256 * side + 128 stays inside the guard band
#define MR_MAX_FACES 16777215  // triangle index + 1 must be exact in float32

struct MrTri {
  int X0, Y0, X1, Y1, X2, Y2;   // snapped, 8 sub-pixel bits
  int sgn;                      // sign of the area
  int64_t area;                 // normalised: > 0
  float zw0, zw1, zw2, w0, w1, w2;
  int i0, i1, i2;               // the vertex indices and the clip-space positions as read
  float4 p0, p1, p2;
};

__device__ __forceinline__ bool mr_snap(float x, float w, int size, int& out) {
  const float ndc = x / w;
  const float s = (ndc * 0.5f + 0.5f) * (float)size;
  const float t = rintf(s * 256.0f);
  if (!(fabsf(t) <= MR_GUARD)) return false;
  out = (int)t;
  return true;
}

// the triangle f of one view as the definition sees it; false: dropped whole
__device__ __forceinline__ bool mr_load(const float* __restrict__ pos, const int32_t* __restrict__ tri, int f, int V, int H, int W,
                                        int cull, MrTri& t) {
  const int i0 = tri[(int64_t)f * 3], i1 = tri[(int64_t)f * 3 + 1], i2 = tri[(int64_t)f * 3 + 2];
  if (i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V) return false;
  const float4 p0 = ((const float4*)pos)[i0], p1 = ((const float4*)pos)[i1], p2 = ((const float4*)pos)[i2];
  if (!(p0.w > 0.f) || !(p1.w > 0.f) || !(p2.w > 0.f)) return false;
  if (!mr_snap(p0.x, p0.w, W, t.X0) || !mr_snap(p0.y, p0.w, H, t.Y0) || !mr_snap(p1.x, p1.w, W, t.X1) ||
      !mr_snap(p1.y, p1.w, H, t.Y1) || !mr_snap(p2.x, p2.w, W, t.X2) || !mr_snap(p2.y, p2.w, H, t.Y2))
    return false;
  const int64_t area = (int64_t)(t.X1 - t.X0) * (t.Y2 - t.Y0) - (int64_t)(t.Y1 - t.Y0) * (t.X2 - t.X0);
  if (area == 0 || (area < 0 && cull)) return false;
  t.sgn = area < 0 ? -1 : 1;
  t.area = area < 0 ? -area : area;
  t.zw0 = p0.z / p0.w;
  t.zw1 = p1.z / p1.w;
  t.zw2 = p2.z / p2.w;
  t.w0 = p0.w;
  t.w1 = p1.w;
  t.w2 = p2.w;
  t.i0 = i0, t.i1 = i1, t.i2 = i2;
  t.p0 = p0, t.p1 = p1, t.p2 = p2;
  return true;
}

// the three normalised edge functions at the point (Px, Py)
__device__ __forceinline__ void mr_edges(const MrTri& t, int Px, int Py, int64_t& e0, int64_t& e1, int64_t& e2) {
  e0 = t.sgn * ((int64_t)(t.X2 - t.X1) * (Py - t.Y1) - (int64_t)(t.Y2 - t.Y1) * (Px - t.X1));
  e1 = t.sgn * ((int64_t)(t.X0 - t.X2) * (Py - t.Y2) - (int64_t)(t.Y0 - t.Y2) * (Px - t.X2));
  e2 = t.sgn * ((int64_t)(t.X1 - t.X0) * (Py - t.Y0) - (int64_t)(t.Y1 - t.Y0) * (Px - t.X0));
}

// the edge functions' steps from one pixel to the next: E(Px + 256, Py) - E(Px, Py) = -256 dy,  E(Px, Py + 256) - E(Px, Py) = 256 dx
__device__ __forceinline__ void mr_steps(const MrTri& t, int64_t& sx0, int64_t& sy0, int64_t& sx1, int64_t& sy1, int64_t& sx2, int64_t& sy2) {
  sx0 = -256 * (int64_t)(t.sgn * (t.Y2 - t.Y1)), sy0 = 256 * (int64_t)(t.sgn * (t.X2 - t.X1));
  sx1 = -256 * (int64_t)(t.sgn * (t.Y0 - t.Y2)), sy1 = 256 * (int64_t)(t.sgn * (t.X0 - t.X2));
  sx2 = -256 * (int64_t)(t.sgn * (t.Y1 - t.Y0)), sy2 = 256 * (int64_t)(t.sgn * (t.X1 - t.X0));
}

__device__ __forceinline__ void mr_weights(const MrTri& t, int64_t e0, int64_t e1, int64_t e2, float& b0, float& b1, float& b2) {
  const float fa = (float)t.area;
  b0 = (float)e0 / fa;
  b1 = (float)e1 / fa;
  b2 = (float)e2 / fa;
}

// the screen-space weights b_i, the perspective weights q_i = b_i / w_i and their sum S = (q0 + q1) + q2 at the centre of pixel (px, py)
struct MrPersp {
  float b0, b1, b2, q0, q1, q2, S;
};

__device__ __forceinline__ MrPersp mr_persp(const MrTri& t, int px, int py) {
  MrPersp r;
  int64_t e0, e1, e2;
  mr_edges(t, 256 * px + 128, 256 * py + 128, e0, e1, e2);
  mr_weights(t, e0, e1, e2, r.b0, r.b1, r.b2);
  r.q0 = r.b0 / t.w0, r.q1 = r.b1 / t.w1, r.q2 = r.b2 / t.w2;
  r.S = (r.q0 + r.q1) + r.q2;
  return r;
}

// pixel g of [B, H, W]: its view, column and row
struct MrPixel {
  int b, px, py;
};

__device__ __forceinline__ MrPixel mr_pixel(int64_t g, int H, int W) {
  MrPixel r;
  r.b = (int)(g / ((int64_t)H * W));
  const int pix = (int)(g - (int64_t)r.b * H * W);
  r.py = pix / W;
  r.px = pix - r.py * W;
  return r;
}

struct MrBil {
  int x0, x1, y0, y1;
  float fx, fy;
};

__device__ __forceinline__ MrBil mr_bilinear(float s, float t, int Th, int Tw) {
  MrBil r;
  const float x = s * (float)Tw - 0.5f, y = t * (float)Th - 0.5f;
  const float xf = floorf(x), yf = floorf(y);
  r.fx = x - xf;
  r.fy = y - yf;
  const int xi = (int)fminf(fmaxf(xf, -1.f), (float)Tw), yi = (int)fminf(fmaxf(yf, -1.f), (float)Th);   // NaN: -1
  r.x0 = min(max(xi, 0), Tw - 1);
  r.x1 = min(max(xi + 1, 0), Tw - 1);
  r.y0 = min(max(yi, 0), Th - 1);
  r.y1 = min(max(yi + 1, 0), Th - 1);
  return r;
}

// One lookup: the bilinear set-up, the offsets (in floats, channel 0) of its four texels inside the buffer that is read or added to, and
// the four texels' weights.  base: where the [Th, Tw, C] texture begins in that buffer.
struct MrTap {
  MrBil q;
  int64_t o00, o01, o10, o11;
  float w00, w01, w10, w11;
};

__device__ __forceinline__ MrTap mr_tap(float s, float t, int Th, int Tw, int C, int64_t base) {
  MrTap r;
  r.q = mr_bilinear(s, t, Th, Tw);
  r.o00 = base + ((int64_t)r.q.y0 * Tw + r.q.x0) * C;
  r.o01 = base + ((int64_t)r.q.y0 * Tw + r.q.x1) * C;
  r.o10 = base + ((int64_t)r.q.y1 * Tw + r.q.x0) * C;
  r.o11 = base + ((int64_t)r.q.y1 * Tw + r.q.x1) * C;
  r.w00 = (1.f - r.q.fy) * (1.f - r.q.fx), r.w01 = (1.f - r.q.fy) * r.q.fx, r.w10 = r.q.fy * (1.f - r.q.fx), r.w11 = r.q.fy * r.q.fx;
  return r;
}

// channel c of the lookup in p
__device__ __forceinline__ float mr_tap_mix(const MrTap& t, const float* p, int c) {
  const float t00 = p[t.o00 + c], t01 = p[t.o01 + c], t10 = p[t.o10 + c], t11 = p[t.o11 + c];
  return (1.f - t.q.fy) * ((1.f - t.q.fx) * t00 + t.q.fx * t01) + t.q.fy * ((1.f - t.q.fx) * t10 + t.q.fx * t11);
}

// the gradient v of channel c to the four texels of g
__device__ __forceinline__ void mr_tap_scatter(const MrTap& t, float* g, int c, float v) {
  atomicAdd(g + t.o00 + c, t.w00 * v);
  atomicAdd(g + t.o01 + c, t.w01 * v);
  atomicAdd(g + t.o10 + c, t.w10 * v);
  atomicAdd(g + t.o11 + c, t.w11 * v);
}

// v times channel c's slopes in x and y (per texel: the caller scales by the sides) added to gs and gt
__device__ __forceinline__ void mr_tap_slopes(const MrTap& t, const float* p, int c, float v, float& gs, float& gt) {
  const float t00 = p[t.o00 + c], t01 = p[t.o01 + c], t10 = p[t.o10 + c], t11 = p[t.o11 + c];
  gs += v * ((1.f - t.q.fy) * (t01 - t00) + t.q.fy * (t11 - t10));
  gt += v * ((1.f - t.q.fx) * (t10 - t00) + t.q.fx * (t11 - t01));
}

__device__ __forceinline__ float mr_interp(float u, float v, float w, float a0, float a1, float a2) { return (u * a0 + v * a1) + w * a2; }

// The fused shade's set-up at a pixel of triangle f with rast value r: the face's six uv values a, the three v after flip_v, w = (1 - u) - v
// and the interpolated (s, t) to look up.
struct MrShade {
  const float* a;
  float v0, v1, v2, w, s, t;
};

__device__ __forceinline__ MrShade mr_shade(const float4& r, const float* uv, int f, int flip_v) {
  MrShade h;
  h.a = uv + (int64_t)f * 6;
  h.w = (1.f - r.x) - r.y;
  h.v0 = flip_v ? 1.f - h.a[1] : h.a[1], h.v1 = flip_v ? 1.f - h.a[3] : h.a[3], h.v2 = flip_v ? 1.f - h.a[5] : h.a[5];
  h.s = mr_interp(r.x, r.y, h.w, h.a[0], h.a[2], h.a[4]);
  h.t = mr_interp(r.x, r.y, h.w, h.v0, h.v1, h.v2);
  return h;
}

// the three rows of attr that the pixel's triangle names; false at an empty pixel or a triangle / row out of range
__device__ __forceinline__ bool mr_corners(const float4& r, const int32_t* __restrict__ idx, int F, int N, int64_t& i0, int64_t& i1,
                                           int64_t& i2) {
  const int f = (int)r.w - 1;
  if (f < 0 || f >= F) return false;
  if (idx) {
    i0 = idx[(int64_t)f * 3];
    i1 = idx[(int64_t)f * 3 + 1];
    i2 = idx[(int64_t)f * 3 + 2];
  } else {
    i0 = (int64_t)f * 3;
    i1 = i0 + 1;
    i2 = i0 + 2;
  }
  return i0 >= 0 && i0 < N && i1 >= 0 && i1 < N && i2 >= 0 && i2 < N;
}

static int mr_image_ok(int32_t B, int32_t H, int32_t W) {
  return B >= 1 && H >= 1 && W >= 1 && H <= MR_MAX_SIZE && W <= MR_MAX_SIZE && (int64_t)B * H * W <= INT32_MAX;
}

// the shapes shared by the per-pixel entry points: pixels = B * H * W of rast / uv, a batch of 1 or B on the other operand
static int mr_batch_ok(int32_t B, int32_t H, int32_t W, int32_t batch) { return mr_image_ok(B, H, W) && (batch == 1 || batch == B); }

// the stride from one view's part of a batched operand of n floats a view to the next: 0 where one part serves every view
static int64_t mr_stride(int32_t batch, int64_t n) { return batch == 1 ? 0 : n; }

static int mr_mesh_ok(int32_t B, int64_t V, int64_t F, int32_t H, int32_t W) {
  return mr_image_ok(B, H, W) && V >= 0 && V <= INT32_MAX && F >= 0 && F <= MR_MAX_FACES;
}

// rows [attr_batch, N, C] at the corners idx [F, 3] names (no idx: face-varying, N = 3 F); absent only where no pixel can name one
static int mr_attr_ok(const float* rows, int32_t attr_batch, int64_t N, int32_t C, const int32_t* idx, int64_t F, int32_t B, int32_t H, int32_t W) {
  return mr_batch_ok(B, H, W, attr_batch) && N >= 0 && N <= INT32_MAX && C >= 1 && F >= 0 && F <= MR_MAX_FACES && (idx || N == 3 * F) &&
         N * C <= INT32_MAX && (rows || F == 0 || N == 0);
}

static int mr_tex_ok(int32_t Th, int32_t Tw, int32_t C) {
  return Th >= 1 && Tw >= 1 && C >= 1 && Th <= MR_MAX_SIZE && Tw <= MR_MAX_SIZE && (int64_t)Th * Tw * C <= INT32_MAX;
}
