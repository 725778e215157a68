// mesh_raster_common.h — the device helpers that mesh_raster.hip (the forward, the attribute and texture gradients) and mesh_grad.hip
// (the gradients to positions, the antialias pass) share: a triangle as the definition of mesh_raster.hip's header sees it, the
// attribute rows a pixel's triangle names, and the bilinear lookup's set-up.  Both files are compiled with -ffp-contract=off; every function here is inlined.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gip_model.h"

#define MR_THREADS 256
#define MR_GUARD 4194304.f     // 2^22: the guard band of snapped coordinates
#define MR_MAX_SIZE 16384      // image side: 256 * side + 128 stays inside the guard band
#define MR_MAX_FACES 16777215  // triangle index + 1 must be exact in float32

struct MrTri {
  int X0, Y0, X1, Y1, X2, Y2;   // snapped, 8 sub-pixel bits
  int sgn;                      // sign of the area
  int64_t area;                 // normalised: > 0
  float zw0, zw1, zw2, w0, w1, w2;
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
  return true;
}

// the three normalised edge functions at the point (Px, Py)
__device__ __forceinline__ void mr_edges(const MrTri& t, int Px, int Py, int64_t& e0, int64_t& e1, int64_t& e2) {
  e0 = t.sgn * ((int64_t)(t.X2 - t.X1) * (Py - t.Y1) - (int64_t)(t.Y2 - t.Y1) * (Px - t.X1));
  e1 = t.sgn * ((int64_t)(t.X0 - t.X2) * (Py - t.Y2) - (int64_t)(t.Y0 - t.Y2) * (Px - t.X2));
  e2 = t.sgn * ((int64_t)(t.X1 - t.X0) * (Py - t.Y0) - (int64_t)(t.Y1 - t.Y0) * (Px - t.X0));
}

__device__ __forceinline__ void mr_weights(const MrTri& t, int64_t e0, int64_t e1, int64_t e2, float& b0, float& b1, float& b2) {
  const float fa = (float)t.area;
  b0 = (float)e0 / fa;
  b1 = (float)e1 / fa;
  b2 = (float)e2 / fa;
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

__device__ __forceinline__ float mr_mix(const MrBil& r, float t00, float t01, float t10, float t11) {
  return (1.f - r.fy) * ((1.f - r.fx) * t00 + r.fx * t01) + r.fy * ((1.f - r.fx) * t10 + r.fx * t11);
}

__device__ __forceinline__ float mr_interp(float u, float v, float w, float a0, float a1, float a2) { return (u * a0 + v * a1) + w * a2; }

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

static unsigned mr_blocks(int64_t n) { return (unsigned)((n + MR_THREADS - 1) / MR_THREADS); }

static int mr_done(void) { return hipGetLastError() == hipSuccess ? 0 : 3; }

static int mr_tex_ok(int32_t Th, int32_t Tw, int32_t C) {
  return Th >= 1 && Tw >= 1 && C >= 1 && Th <= MR_MAX_SIZE && Tw <= MR_MAX_SIZE && (int64_t)Th * Tw * C <= INT32_MAX;
}
