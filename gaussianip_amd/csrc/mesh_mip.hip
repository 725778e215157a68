// mesh_mip.hip — pixel differentials and the mipmapped texture lookup of the mesh rasterizer: what nvdiffrast calls rast_db, diff_attrs,
// uv_da / mip_level_bias / mip (DESIGN.md "Pixel differentials and mipmaps"; MipMeshRasterizerContext of
// gaussianip_amd/utils/rasterize.py).  Linked into libgip_model.so, compiled with its -ffp-contract=off; the triangle set-up and the
// bilinear rule are those of mesh_raster_common.h, so mesh_raster.hip's definition of a triangle and of a lookup holds here unchanged.
//
// Definitions (tests/mesh_mip_reference.py restates them in numpy; float32, in this operand order, left to right).
//   * rast_db [B, H, W, 4] = (du/dX, du/dY, dv/dX, dv/dY): X, Y in pixels, Y growing with the row index; (u, v) the perspective-correct
//     weights rast holds.  The pixel's triangle as mr_load sees it (snapped, area normalised, no culling: it won the pixel).  The
//     screen-space weights b_i = (float) E_i / (float) area are linear in the pixel:
//       dXb0 = (float) (-256 sgn (Y2 - Y1)) / (float) area,   dYb0 = (float) (256 sgn (X2 - X1)) / (float) area,
//     b1 with (Y0 - Y2, X0 - X2), b2 with (Y1 - Y0, X1 - X0); the integer numerators are int64.  With q_i = b_i / w_i (b_i recomputed
//     as the resolve kernel does), S = (q0 + q1) + q2, dq_i = db_i / w_i and dS = (dq0 + dq1) + dq2 per axis:
//       du = (dq0 - u * dS) / S,   dv = (dq1 - v * dS) / S,   u and v read from rast.
//     All zeros at an empty pixel, where the triangle index is out of range and where mr_load drops the triangle.  No gradient
//     reaches pos through rast_db (nvdiffrast's grad_db = False).
//   * Attribute differentials: for channel c of the pixel's three corner rows a0, a1, a2 (mr_corners),
//       da/dX = du/dX * (a0 - a2) + dv/dX * (a1 - a2),   da/dY = du/dY * (a0 - a2) + dv/dY * (a1 - a2),
//     out_da [B, H, W, 2 K] = (da/dX, da/dY) of the K listed channels in the list's order (no list: all C channels), zeros at an
//     empty pixel.  Backward, per listed channel with upstream (gX, gY): g0 = du/dX * gX + du/dY * gY to row i0, g1 = dv/dX * gX +
//     dv/dY * gY to row i1, -(g0 + g1) to row i2, float atomic adds.  out_da does not depend on (u, v): nothing reaches rast.
//   * Mip stack of a texture [Th, Tw, C]: level l + 1 has sides max(side_l / 2, 1); a texel is ((t00 + t01) + (t10 + t11)) * 0.25f of
//     its 2 x 2 block in level l (t00 t01 the upper row), and (a + b) * 0.5f of its pair where one side of level l is already 1.  A
//     level is built only while every side greater than 1 is even; the stack ends at 1 x 1, at the first level with an odd side
//     greater than 1, or at max_level (negative: no cap), whichever comes first.  L is the last level's index; L = 0 is legal.  Level
//     0 is the texture itself; the buffer `mip` holds levels 1 .. L one after the other, mip_texels texels of C floats per texture.
//   * Level of detail (nvdiffrast's rule), level 0 of sides Tw, Th, uv_da = (ds/dX, ds/dY, dt/dX, dt/dY):
//       sx = uv_da.x * Tw,  sy = uv_da.y * Tw,  tx = uv_da.z * Th,  ty = uv_da.w * Th,
//       A = sx * sx + tx * tx,  B = sy * sy + ty * ty,  Cc = sx * sy + tx * ty,  D = A - B,
//       R = sqrtf(0.25f * (D * D) + Cc * Cc),  m = 0.5f * (A + B) + R,  level = 0.5f * log2f(m) + bias
//     (without uv_da: level = bias; without a bias: bias = 0).  lc = fminf(fmaxf(level, 0), L): a NaN counts as 0.
//   * Trilinear: l0 = floorf(lc), f = lc - l0, l1 = min(l0 + 1, L), out = (1 - f) * bil_l0 + f * bil_l1 with bil_l the bilinear rule
//     (mr_bilinear, mr_tap_mix) on level l's sides; where f == 0 only level l0 is read and out = bil_l0 itself.  Mipmap-nearest:
//     l0 = min((int) floorf(lc + 0.5f), L), f = 0.
//   * Gradients, per channel with upstream v: gv0 = (1 - f) * v and gv1 = f * v take the place of the upstream gradient in the
//     bilinear rule's gradients at levels l0 and l1 (to the four texels: float atomic adds into a gradient stack of the same layout; to
//     uv: (gs0 * Tw_l0 + gs1 * Tw_l1, gt0 * Th_l0 + gt1 * Th_l1)).  dL/dlevel = sum_c v * (bil_l1 - bil_l0) where 0 < level < L strictly
//     and the mode is trilinear, else 0 (at an integer level inside that range l1 = l0 + 1 is read for it); this is dL/dbias.
//     dL/duv_da = dL/dlevel * 0.5f / (m * ln 2) * (dm/dsx * Tw, dm/dsy * Tw, dm/dtx * Th, dm/dty * Th) with mA = 0.5f + 0.25f * D / R,
//     mB = 0.5f - 0.25f * D / R, mC = Cc / R (R == 0: 0.5, 0.5, 0), dm/dsx = mA * (2 sx) + mC * sy, dm/dsy = mB * (2 sy) + mC * sx,
//     dm/dtx = mA * (2 tx) + mC * ty, dm/dty = mB * (2 ty) + mC * tx; zeros where m == 0 or dL/dlevel is 0 by the rule above.
//   * The fold: the gradient stack goes to level 0 top-down by the transpose of the build, g_l[texel] += 0.25f (or 0.5f) *
//     g_(l+1)[its parent]: a gather, one launch per level, bit-reproducible given the stack.
//
//   mesh_rast_db_kernel               one lane per pixel: one 16-byte load of rast, the triangle's three float4 positions, one 16-byte store.
//   mesh_interpolate_da_kernel        one lane per pixel, any K.
//   mesh_interpolate_da_backward_kernel   one lane per pixel: 3 float atomic adds per listed channel.
//   mesh_mip_build_kernel             one lane per float of level l + 1 (all textures of the batch in one launch); one launch per level.
//   mesh_mip_fold_kernel              one lane per float of level l; one launch per level, from level L - 1 down to 0.
//   mesh_texture_mip_kernel           one lane per pixel: uv_da as one float4, the level's sides and offset computed in registers (a
//                                     loop of at most 14 trips), four texels per channel at l0 and four more at l1 where f != 0.
//   mesh_texture_mip_backward_kernel  one lane per pixel: up to 8 float atomic adds per channel, g_uv / g_uv_da / g_bias stored per pixel.
#include "mesh_raster_common.h"

#define MM_MAX_LEVEL 14   // 16384 = 2^14 texels a side at most

// ------------------------------------------------------------------------------------------------------------------ rast_db
__global__ void __launch_bounds__(MR_THREADS)
mesh_rast_db_kernel(const float* __restrict__ pos, const int32_t* __restrict__ tri, int B, int V, int F, int H, int W,
                    const float4* __restrict__ rast, float4* __restrict__ rast_db) {
  const int64_t g = (int64_t)blockIdx.x * MR_THREADS + threadIdx.x;
  if (g >= (int64_t)B * H * W) return;
  const float4 r = rast[g];
  float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
  const int f = (int)r.w - 1;
  if (f >= 0 && f < F) {
    const MrPixel p = mr_pixel(g, H, W);
    MrTri t;
    if (mr_load(pos + (int64_t)p.b * V * 4, tri, f, V, H, W, 0, t)) {
      const float S = mr_persp(t, p.px, p.py).S;
      int64_t sx0, sy0, sx1, sy1, sx2, sy2;
      mr_steps(t, sx0, sy0, sx1, sy1, sx2, sy2);
      const float fa = (float)t.area;
      const float bx0 = (float)sx0 / fa, by0 = (float)sy0 / fa;
      const float bx1 = (float)sx1 / fa, by1 = (float)sy1 / fa;
      const float bx2 = (float)sx2 / fa, by2 = (float)sy2 / fa;
      const float qx0 = bx0 / t.w0, qx1 = bx1 / t.w1, qx2 = bx2 / t.w2;
      const float qy0 = by0 / t.w0, qy1 = by1 / t.w1, qy2 = by2 / t.w2;
      const float Sx = (qx0 + qx1) + qx2, Sy = (qy0 + qy1) + qy2;
      out = make_float4((qx0 - r.x * Sx) / S, (qy0 - r.x * Sy) / S, (qx1 - r.y * Sx) / S, (qy1 - r.y * Sy) / S);
    }
  }
  rast_db[g] = out;
}

// ------------------------------------------------------------------------------------------------------------------ attribute differentials
// the channel the k-th pair of out_da belongs to; -1: outside [0, C) (nothing is read for it)
__device__ __forceinline__ int mm_channel(const int32_t* __restrict__ channels, int k, int C) {
  const int c = channels ? channels[k] : k;
  return (c >= 0 && c < C) ? c : -1;
}

__global__ void __launch_bounds__(MR_THREADS)
mesh_interpolate_da_kernel(const float* __restrict__ attr, int64_t attr_stride, const int32_t* __restrict__ idx, const float4* __restrict__ rast,
                           const float4* __restrict__ rast_db, const int32_t* __restrict__ channels, int K, int64_t pixels, int64_t per_view,
                           int F, int N, int C, float2* __restrict__ out_da) {
  const int64_t g = (int64_t)blockIdx.x * MR_THREADS + threadIdx.x;
  if (g >= pixels) return;
  const float4 r = rast[g];
  float2* o = out_da + g * K;
  int64_t i0, i1, i2;
  if (!mr_corners(r, idx, F, N, i0, i1, i2)) {
    for (int k = 0; k < K; k++) o[k] = make_float2(0.f, 0.f);
    return;
  }
  const float4 d = rast_db[g];
  const float* a = attr + (g / per_view) * attr_stride;
  for (int k = 0; k < K; k++) {
    const int c = mm_channel(channels, k, C);
    float2 v = make_float2(0.f, 0.f);
    if (c >= 0) {
      const float a2 = a[i2 * C + c];
      const float d0 = a[i0 * C + c] - a2, d1 = a[i1 * C + c] - a2;
      v = make_float2(d.x * d0 + d.z * d1, d.y * d0 + d.w * d1);
    }
    o[k] = v;
  }
}

__global__ void __launch_bounds__(MR_THREADS)
mesh_interpolate_da_backward_kernel(const float2* __restrict__ g_da, const int32_t* __restrict__ idx, const float4* __restrict__ rast,
                                    const float4* __restrict__ rast_db, const int32_t* __restrict__ channels, int K, int64_t pixels,
                                    int64_t per_view, int F, int N, int C, float* __restrict__ g_attr, int64_t attr_stride) {
  const int64_t g = (int64_t)blockIdx.x * MR_THREADS + threadIdx.x;
  if (g >= pixels) return;
  const float4 r = rast[g];
  int64_t i0, i1, i2;
  if (!mr_corners(r, idx, F, N, i0, i1, i2)) return;
  const float4 d = rast_db[g];
  float* a = g_attr + (g / per_view) * attr_stride;
  const float2* go = g_da + g * K;
  for (int k = 0; k < K; k++) {
    const int c = mm_channel(channels, k, C);
    if (c < 0) continue;
    const float2 v = go[k];
    const float g0 = d.x * v.x + d.y * v.y, g1 = d.z * v.x + d.w * v.y;
    atomicAdd(a + i0 * C + c, g0);
    atomicAdd(a + i1 * C + c, g1);
    atomicAdd(a + i2 * C + c, -(g0 + g1));
  }
}

// ------------------------------------------------------------------------------------------------------------------ the mip stack
// L and the texels of levels 1 .. L of a Th x Tw texture; max_level < 0: no cap
static void mm_levels(int Th, int Tw, int max_level, int& L, int64_t& texels) {
  L = 0;
  texels = 0;
  int h = Th, w = Tw;
  while ((h > 1 || w > 1) && (max_level < 0 || L < max_level) && (h == 1 || h % 2 == 0) && (w == 1 || w % 2 == 0)) {
    h = h > 1 ? h / 2 : 1;
    w = w > 1 ? w / 2 : 1;
    texels += (int64_t)h * w;
    L++;
  }
}

// level l (0 .. L) of the stack: its sides and, for l >= 1, its offset in texels inside `mip`
struct MmLevel {
  int h, w;
  int64_t off;
};

__host__ __device__ __forceinline__ MmLevel mm_level(int Th, int Tw, int l) {
  MmLevel r;
  r.h = Th;
  r.w = Tw;
  r.off = 0;
  for (int i = 0; i < l; i++) {
    if (i > 0) r.off += (int64_t)r.h * r.w;
    r.h = r.h > 1 ? r.h >> 1 : 1;
    r.w = r.w > 1 ? r.w >> 1 : 1;
  }
  return r;
}

// dst [nb, h2, w2, C] (level l + 1) from src [nb, h, w, C] (level l); n = nb * h2 * w2 * C
__global__ void __launch_bounds__(MR_THREADS)
mesh_mip_build_kernel(const float* __restrict__ src, int64_t src_stride, float* __restrict__ dst, int64_t dst_stride, int h, int w, int C,
                      int64_t n) {
  const int64_t g = (int64_t)blockIdx.x * MR_THREADS + threadIdx.x;
  if (g >= n) return;
  const int h2 = h > 1 ? h >> 1 : 1, w2 = w > 1 ? w >> 1 : 1;
  const int64_t per = (int64_t)h2 * w2 * C;
  const int64_t b = g / per, i = g - b * per;
  const int c = (int)(i % C);
  const int64_t texel = i / C;
  const int y = (int)(texel / w2), x = (int)(texel - (int64_t)y * w2);
  const float* s = src + b * src_stride + c;
  float v;
  if (h > 1 && w > 1) {
    const float* p = s + ((int64_t)(2 * y) * w + 2 * x) * C;
    v = ((p[0] + p[C]) + (p[(int64_t)w * C] + p[(int64_t)w * C + C])) * 0.25f;
  } else if (h > 1) {      // w == 1: a column
    v = (s[(int64_t)(2 * y) * C] + s[(int64_t)(2 * y + 1) * C]) * 0.5f;
  } else {                 // h == 1: a row
    v = (s[(int64_t)(2 * x) * C] + s[(int64_t)(2 * x + 1) * C]) * 0.5f;
  }
  dst[b * dst_stride + i] = v;
}

// g_lo [nb, h, w, C] (level l) += the share of g_hi [nb, h2, w2, C] (level l + 1): the transpose of the build; n = nb * h * w * C
__global__ void __launch_bounds__(MR_THREADS)
mesh_mip_fold_kernel(float* __restrict__ g_lo, int64_t lo_stride, const float* __restrict__ g_hi, int64_t hi_stride, int h, int w, int C,
                     int64_t n) {
  const int64_t g = (int64_t)blockIdx.x * MR_THREADS + threadIdx.x;
  if (g >= n) return;
  const int w2 = w > 1 ? w >> 1 : 1;
  const int64_t per = (int64_t)h * w * C;
  const int64_t b = g / per, i = g - b * per;
  const int c = (int)(i % C);
  const int64_t texel = i / C;
  const int y = (int)(texel / w), x = (int)(texel - (int64_t)y * w);
  const int py = h > 1 ? y >> 1 : 0, px = w > 1 ? x >> 1 : 0;
  const float share = (h > 1 && w > 1) ? 0.25f : 0.5f;
  g_lo[b * lo_stride + i] += share * g_hi[b * hi_stride + ((int64_t)py * w2 + px) * C + c];
}

// ------------------------------------------------------------------------------------------------------------------ the mipmapped lookup
struct MmLod {
  float level;                  // before the clamp
  float sx, sy, tx, ty, D, Cc, R, m;
};

__device__ __forceinline__ MmLod mm_lod(const float4* __restrict__ uv_da, const float* __restrict__ bias, int64_t g, int Th, int Tw) {
  MmLod r;
  r.sx = r.sy = r.tx = r.ty = r.D = r.Cc = r.R = r.m = 0.f;
  r.level = bias ? bias[g] : 0.f;
  if (uv_da) {
    const float4 d = uv_da[g];
    r.sx = d.x * (float)Tw;
    r.sy = d.y * (float)Tw;
    r.tx = d.z * (float)Th;
    r.ty = d.w * (float)Th;
    const float A = r.sx * r.sx + r.tx * r.tx, B = r.sy * r.sy + r.ty * r.ty;
    r.Cc = r.sx * r.sy + r.tx * r.ty;
    r.D = A - B;
    r.R = sqrtf(0.25f * (r.D * r.D) + r.Cc * r.Cc);
    r.m = 0.5f * (A + B) + r.R;
    r.level = 0.5f * log2f(r.m) + r.level;
  }
  return r;
}

// the two levels and the weight of the second; f == 0: only l0 is read
__device__ __forceinline__ void mm_select(float level, int L, int nearest, int& l0, int& l1, float& f) {
  const float lc = fminf(fmaxf(level, 0.f), (float)L);      // NaN: 0
  if (nearest) {
    l0 = min((int)floorf(lc + 0.5f), L);
    l1 = l0;
    f = 0.f;
  } else {
    const float fl = floorf(lc);
    l0 = min(max((int)fl, 0), L);
    l1 = min(l0 + 1, L);
    f = lc - fl;
  }
}

// the lookup at level l, which is lv, inside its buffer (tex for l == 0, mip above)
__device__ __forceinline__ MrTap mm_tap(float2 st, const MmLevel& lv, int l, int C, int64_t tex_base, int64_t mip_base) {
  return mr_tap(st.x, st.y, lv.h, lv.w, C, l == 0 ? tex_base : mip_base + lv.off * C);
}

__global__ void __launch_bounds__(MR_THREADS)
mesh_texture_mip_kernel(const float* __restrict__ tex, int64_t tex_stride, const float* __restrict__ mip, int64_t mip_stride,
                        const float2* __restrict__ uv, const float4* __restrict__ uv_da, const float* __restrict__ bias, int64_t pixels,
                        int64_t per_view, int Th, int Tw, int C, int L, int nearest, float* __restrict__ out) {
  const int64_t g = (int64_t)blockIdx.x * MR_THREADS + threadIdx.x;
  if (g >= pixels) return;
  const float2 st = uv[g];
  const MmLod lod = mm_lod(uv_da, bias, g, Th, Tw);
  int l0, l1;
  float f;
  mm_select(lod.level, L, nearest, l0, l1, f);
  const int64_t b = g / per_view;
  const MrTap t0 = mm_tap(st, mm_level(Th, Tw, l0), l0, C, b * tex_stride, b * mip_stride);
  const float* p0 = l0 == 0 ? tex : mip;
  float* o = out + g * C;
  if (f == 0.f) {
    for (int c = 0; c < C; c++) o[c] = mr_tap_mix(t0, p0, c);
    return;
  }
  const MrTap t1 = mm_tap(st, mm_level(Th, Tw, l1), l1, C, b * tex_stride, b * mip_stride);      // f != 0: l1 = l0 + 1 >= 1
  for (int c = 0; c < C; c++) {
    o[c] = (1.f - f) * mr_tap_mix(t0, p0, c) + f * mr_tap_mix(t1, mip, c);
  }
}

__global__ void __launch_bounds__(MR_THREADS)
mesh_texture_mip_backward_kernel(const float* __restrict__ tex, int64_t tex_stride, const float* __restrict__ mip, int64_t mip_stride,
                                 const float2* __restrict__ uv, const float4* __restrict__ uv_da, const float* __restrict__ bias,
                                 const float* __restrict__ g_out, int64_t pixels, int64_t per_view, int Th, int Tw, int C, int L, int nearest,
                                 float* __restrict__ g_tex, float* __restrict__ g_mip, float2* __restrict__ g_uv, float4* __restrict__ g_uv_da,
                                 float* __restrict__ g_bias) {
  const int64_t g = (int64_t)blockIdx.x * MR_THREADS + threadIdx.x;
  if (g >= pixels) return;
  const float2 st = uv[g];
  const MmLod lod = mm_lod(uv_da, bias, g, Th, Tw);
  int l0, l1;
  float f;
  mm_select(lod.level, L, nearest, l0, l1, f);
  // dL/dlevel is taken where the level moves freely: strictly inside (0, L), trilinear, and asked for
  const bool gate = !nearest && (g_uv_da || g_bias) && lod.level > 0.f && lod.level < (float)L;
  const bool second = f != 0.f || gate;      // then l1 = l0 + 1 <= L
  const int64_t b = g / per_view;
  const MmLevel v0 = mm_level(Th, Tw, l0), v1 = mm_level(Th, Tw, second ? l1 : l0);
  const MrTap t0 = mm_tap(st, v0, l0, C, b * tex_stride, b * mip_stride);
  const MrTap t1 = mm_tap(st, v1, second ? l1 : l0, C, b * tex_stride, b * mip_stride);
  const float* p0 = l0 == 0 ? tex : mip;
  float* a0 = l0 == 0 ? g_tex : g_mip;
  const float* go = g_out + g * C;
  const bool values = g_uv || gate;
  float gs0 = 0.f, gt0 = 0.f, gs1 = 0.f, gt1 = 0.f, dl = 0.f;
  for (int c = 0; c < C; c++) {
    const float v = go[c];
    const float gv0 = (1.f - f) * v, gv1 = f * v;
    if (g_tex) {
      mr_tap_scatter(t0, a0, c, gv0);
      if (f != 0.f) mr_tap_scatter(t1, g_mip, c, gv1);
    }
    if (values) {
      mr_tap_slopes(t0, p0, c, gv0, gs0, gt0);
      if (second) {
        mr_tap_slopes(t1, mip, c, gv1, gs1, gt1);
        if (gate) dl += v * (mr_tap_mix(t1, mip, c) - mr_tap_mix(t0, p0, c));
      }
    }
  }
  if (g_uv) g_uv[g] = make_float2(gs0 * (float)v0.w + gs1 * (float)v1.w, gt0 * (float)v0.h + gt1 * (float)v1.h);
  if (g_bias) g_bias[g] = dl;
  if (g_uv_da) {
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (gate && uv_da && lod.m > 0.f) {
      const float k = dl * 0.5f / (lod.m * 0.69314718055994530942f);
      float mA = 0.5f, mB = 0.5f, mC = 0.f;
      if (lod.R > 0.f) {
        const float e = 0.25f * lod.D / lod.R;
        mA = 0.5f + e;
        mB = 0.5f - e;
        mC = lod.Cc / lod.R;
      }
      o.x = k * ((mA * (2.f * lod.sx) + mC * lod.sy) * (float)Tw);
      o.y = k * ((mB * (2.f * lod.sy) + mC * lod.sx) * (float)Tw);
      o.z = k * ((mA * (2.f * lod.tx) + mC * lod.ty) * (float)Th);
      o.w = k * ((mB * (2.f * lod.ty) + mC * lod.tx) * (float)Th);
    }
    g_uv_da[g] = o;
  }
}

// ------------------------------------------------------------------------------------------------------------------ C-ABI
extern "C" int gip_mesh_rast_db(const float* pos, const int32_t* tri, int32_t B, int64_t V, int64_t F, int32_t H, int32_t W, const float* rast,
                                float* rast_db, void* stream) {
  if (!mr_mesh_ok(B, V, F, H, W) || !rast || !rast_db) return 1;
  hipStream_t st = (hipStream_t)stream;
  const int64_t pixels = (int64_t)B * H * W;
  if (F == 0 || V == 0) return hipMemsetAsync(rast_db, 0, (size_t)pixels * 16, st) == hipSuccess ? 0 : 3;
  if (!pos || !tri) return 1;
  hipLaunchKernelGGL(mesh_rast_db_kernel, dim3(mesh_blocks(pixels)), dim3(MR_THREADS), 0, st, pos, tri, (int)B, (int)V, (int)F, (int)H, (int)W,
                     (const float4*)rast, (float4*)rast_db);
  return mesh_done();
}

static int mm_attr_ok(const float* rows, int32_t attr_batch, int64_t N, int32_t C, const int32_t* idx, int64_t F, int32_t K, int32_t B, int32_t H,
                      int32_t W) {
  return mr_attr_ok(rows, attr_batch, N, C, idx, F, B, H, W) && K >= 1 && (int64_t)B * H * W * K * 2 <= INT32_MAX;
}

extern "C" int gip_mesh_interpolate_da(const float* attr, int32_t attr_batch, int64_t N, int32_t C, const int32_t* idx, int64_t F,
                                       const float* rast, const float* rast_db, const int32_t* channels, int32_t K, int32_t B, int32_t H,
                                       int32_t W, float* out_da, void* stream) {
  if (!mm_attr_ok(attr, attr_batch, N, C, idx, F, K, B, H, W) || !rast || !rast_db || !out_da) return 1;
  const int64_t pixels = (int64_t)B * H * W;
  hipLaunchKernelGGL(mesh_interpolate_da_kernel, dim3(mesh_blocks(pixels)), dim3(MR_THREADS), 0, (hipStream_t)stream, attr,
                     mr_stride(attr_batch, N * C), idx, (const float4*)rast, (const float4*)rast_db, channels, (int)K, pixels,
                     (int64_t)H * W, (int)F, (int)N, (int)C, (float2*)out_da);
  return mesh_done();
}

extern "C" int gip_mesh_interpolate_da_backward(const float* g_da, int32_t attr_batch, int64_t N, int32_t C, const int32_t* idx, int64_t F,
                                                const float* rast, const float* rast_db, const int32_t* channels, int32_t K, int32_t B,
                                                int32_t H, int32_t W, float* g_attr, void* stream) {
  if (!mm_attr_ok(g_attr, attr_batch, N, C, idx, F, K, B, H, W) || !rast || !rast_db || !g_da) return 1;
  if (N == 0) return 0;
  if (!g_attr) return 1;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(g_attr, 0, (size_t)attr_batch * N * C * sizeof(float), st) != hipSuccess) return 3;
  const int64_t pixels = (int64_t)B * H * W;
  hipLaunchKernelGGL(mesh_interpolate_da_backward_kernel, dim3(mesh_blocks(pixels)), dim3(MR_THREADS), 0, st, (const float2*)g_da, idx,
                     (const float4*)rast, (const float4*)rast_db, channels, (int)K, pixels, (int64_t)H * W, (int)F, (int)N, (int)C, g_attr,
                     mr_stride(attr_batch, N * C));
  return mesh_done();
}

extern "C" int gip_mesh_mip_levels(int32_t Th, int32_t Tw, int32_t max_level, int32_t* levels, int64_t* texels) {
  if (!mr_tex_ok(Th, Tw, 1) || !levels || !texels) return 1;
  int L;
  int64_t n;
  mm_levels(Th, Tw, max_level, L, n);
  *levels = L;
  *texels = n;
  return 0;
}

// the stack's shape as the caller must have sized it: false when mip_texels is not what (Th, Tw, max_level) gives
static int mm_stack_ok(int32_t tex_batch, int32_t Th, int32_t Tw, int32_t C, int32_t max_level, int64_t mip_texels, int& L) {
  if (!mr_tex_ok(Th, Tw, C) || tex_batch < 1) return 0;
  int64_t n;
  mm_levels(Th, Tw, max_level, L, n);
  return L <= MM_MAX_LEVEL && n == mip_texels && (int64_t)tex_batch * Th * Tw * C <= INT32_MAX;
}

extern "C" int gip_mesh_mip_build(const float* tex, int32_t tex_batch, int32_t Th, int32_t Tw, int32_t C, int32_t max_level, float* mip,
                                  int64_t mip_texels, void* stream) {
  int L;
  if (!mm_stack_ok(tex_batch, Th, Tw, C, max_level, mip_texels, L) || !tex) return 1;
  if (L == 0) return 0;
  if (!mip) return 1;
  for (int l = 0; l < L; l++) {
    const MmLevel lo = mm_level(Th, Tw, l), hi = mm_level(Th, Tw, l + 1);
    const int64_t n = (int64_t)tex_batch * hi.h * hi.w * C;
    hipLaunchKernelGGL(mesh_mip_build_kernel, dim3(mesh_blocks(n)), dim3(MR_THREADS), 0, (hipStream_t)stream,
                       l == 0 ? tex : (const float*)(mip + lo.off * C), l == 0 ? (int64_t)Th * Tw * C : mip_texels * C, mip + hi.off * C,
                       mip_texels * C, lo.h, lo.w, (int)C, n);
  }
  return mesh_done();
}

extern "C" int gip_mesh_mip_fold(float* g_tex, int32_t tex_batch, int32_t Th, int32_t Tw, int32_t C, int32_t max_level, float* g_mip,
                                 int64_t mip_texels, void* stream) {
  int L;
  if (!mm_stack_ok(tex_batch, Th, Tw, C, max_level, mip_texels, L) || !g_tex) return 1;
  if (L == 0) return 0;
  if (!g_mip) return 1;
  for (int l = L - 1; l >= 0; l--) {
    const MmLevel lo = mm_level(Th, Tw, l), hi = mm_level(Th, Tw, l + 1);
    const int64_t n = (int64_t)tex_batch * lo.h * lo.w * C;
    hipLaunchKernelGGL(mesh_mip_fold_kernel, dim3(mesh_blocks(n)), dim3(MR_THREADS), 0, (hipStream_t)stream,
                       l == 0 ? g_tex : g_mip + lo.off * C, l == 0 ? (int64_t)Th * Tw * C : mip_texels * C,
                       (const float*)(g_mip + hi.off * C), mip_texels * C, lo.h, lo.w, (int)C, n);
  }
  return mesh_done();
}

extern "C" int gip_mesh_texture_mip(const float* tex, int32_t tex_batch, int32_t Th, int32_t Tw, int32_t C, const float* mip,
                                    int64_t mip_texels, int32_t max_level, const float* uv, const float* uv_da, const float* bias,
                                    int32_t nearest, int32_t B, int32_t H, int32_t W, float* out, void* stream) {
  int L;
  if (!mr_batch_ok(B, H, W, tex_batch) || !mm_stack_ok(tex_batch, Th, Tw, C, max_level, mip_texels, L) || !tex || !uv || !out) return 1;
  if (L > 0 && !mip) return 1;
  const int64_t pixels = (int64_t)B * H * W;
  hipLaunchKernelGGL(mesh_texture_mip_kernel, dim3(mesh_blocks(pixels)), dim3(MR_THREADS), 0, (hipStream_t)stream, tex,
                     mr_stride(tex_batch, (int64_t)Th * Tw * C), mip, mr_stride(tex_batch, mip_texels * C), (const float2*)uv,
                     (const float4*)uv_da, bias, pixels, (int64_t)H * W, (int)Th, (int)Tw, (int)C, L, (int)(nearest != 0), out);
  return mesh_done();
}

extern "C" int gip_mesh_texture_mip_backward(const float* tex, int32_t tex_batch, int32_t Th, int32_t Tw, int32_t C, const float* mip,
                                             int64_t mip_texels, int32_t max_level, const float* uv, const float* uv_da, const float* bias,
                                             int32_t nearest, const float* g_out, int32_t B, int32_t H, int32_t W, float* g_tex, float* g_mip,
                                             float* g_uv, float* g_uv_da, float* g_bias, void* stream) {
  int L;
  if (!mr_batch_ok(B, H, W, tex_batch) || !mm_stack_ok(tex_batch, Th, Tw, C, max_level, mip_texels, L) || !tex || !uv || !g_out) return 1;
  if ((L > 0 && !mip) || (g_tex && L > 0 && !g_mip) || (g_uv_da && !uv_da) || (g_bias && !bias)) return 1;
  if (!g_tex && !g_uv && !g_uv_da && !g_bias) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (g_tex && hipMemsetAsync(g_tex, 0, (size_t)tex_batch * Th * Tw * C * sizeof(float), st) != hipSuccess) return 3;
  if (g_tex && L > 0 && hipMemsetAsync(g_mip, 0, (size_t)tex_batch * mip_texels * C * sizeof(float), st) != hipSuccess) return 3;
  const int64_t pixels = (int64_t)B * H * W;
  hipLaunchKernelGGL(mesh_texture_mip_backward_kernel, dim3(mesh_blocks(pixels)), dim3(MR_THREADS), 0, st, tex,
                     mr_stride(tex_batch, (int64_t)Th * Tw * C), mip, mr_stride(tex_batch, mip_texels * C), (const float2*)uv,
                     (const float4*)uv_da, bias, g_out, pixels, (int64_t)H * W, (int)Th, (int)Tw, (int)C, L, (int)(nearest != 0), g_tex,
                     L > 0 ? g_mip : (float*)nullptr, (float2*)g_uv, (float4*)g_uv_da, g_bias);
  return mesh_done();
}
