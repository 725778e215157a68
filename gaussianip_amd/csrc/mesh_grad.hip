// mesh_grad.hip — what lets a loss on the rendered mesh reach its geometry: the backward of the rasterizer and of the interpolation into
// clip-space positions, and the antialias pass with its backward (DESIGN.md "Rendering the mesh").  The forward these differentiate is
// mesh_raster.hip's, whose header states coverage, visibility and the weights; mesh_raster_common.h holds the shared set-up.  Linked into
// libgip_model.so, compiled with its -ffp-contract=off.  tests/mesh_grad_reference.py restates everything below in numpy.
//
// Gradient of rast to pos (mesh_rasterize_backward_kernel, one lane per pixel, 12 float atomic adds per covered pixel into the zeroed
// g_pos [B, V, 4]: not bit-reproducible).
//   * The function differentiated is the forward's definition with the snapped integers read as real numbers: sx_i = X_i / 256,
//     sy_i = Y_i / 256 stand for sx = (x / w * 0.5 + 0.5) * W and sy = (y / w * 0.5 + 0.5) * H, the rounding having derivative 1
//     (straight-through): dsx/dx = 0.5 W / w, dsx/dw = -0.5 W (x / w) / w, the same in y with H.
//   * b_i = E_i / area at the pixel centre c.  The gradient of b_i in c, in pixels, is n_i = 256 sign(area) (Y_j - Y_k, X_k - X_j) / area
//     for (i, j, k) a cyclic shift of (0, 1, 2), and moving corner j by a vector m moves every b_i as moving c by -b_j m does:
//     db_i / d(sx_j, sy_j) = -b_j n_i.
//   * q_i = b_i / w_i, S = (q0 + q1) + q2, u = q0 / S, v = q1 / S, d = sum b_i (z_i / w_i).  With (g_u, g_v, g_d) = g_rast[0:3] (channel
//     3 is ignored: the triangle index has no gradient) and k = g_u u + g_v v:  dL/dq = ((g_u - k) / S, (g_v - k) / S, -k / S),
//     dL/db_i = dL/dq_i / w_i + g_d z_i / w_i, G = sum_i dL/db_i n_i, dL/d(sx_j, sy_j) = -b_j G, dL/dz_j = g_d b_j / w_j.
//   * w_j enters three ways and all are in dL/dw_j: through q_j (-dL/dq_j q_j / w_j), through z_j / w_j (-g_d b_j (z_j / w_j) / w_j) and
//     through the screen position (above).
//   * Every lane adds on its own; lanes of a wavefront that share a triangle are not reduced before the atomics.  That reduction is not
//     built: profiles/mesh_grad.json, positions.entry_points.gip_mesh_rasterize_backward, is the figure it would have to beat.
//
// Gradient of interpolated values to rast (mesh_interpolate_backward_rast_kernel, mesh_shade_backward_rast_kernel: one lane per pixel,
// no atomics, one 16-byte store): a = (u a0 + v a1) + ((1 - u) - v) a2 gives g_u = sum_c g_c (a0_c - a2_c), g_v = sum_c g_c (a1_c - a2_c);
// stored as (g_u, g_v, 0, 0), zeros at an empty pixel.  For the fused shade, a is the face's uv (every v replaced by 1 - v first under
// flip_v) and g_c is the lookup's dL/d(s, t) = (Tw sum_c g_c d/dx, Th sum_c g_c d/dy) of mesh_raster.hip's bilinear rule.
//
// The antialias pass (nvdiffrast's rule, every decision in exact integers of the snapped coordinates, as coverage is).
//   * topo [F, 3] int32 (gaussianip_amd.utils.rasterize.edge_topology): for edge k of face f, which is the edge opposite corner k
//     (the numbering of E_k), the vertex of the one other face at that edge that is not on it; -1 when there is no other face; -2 when
//     more than two faces share the edge.  Any other value outside [0, V) reads as -2.
//   * A pair is two horizontally or vertically adjacent pixels of one view whose triangle ids (rast[..., 3]) differ.  The near pixel N
//     is the one that has a triangle; the one with the smaller rast[..., 2] when both have one; at equal depth the one with the lower
//     id.  O is the other pixel, T is N's triangle.  A T that is out of range or not drawn under this pos ends the pair.
//   * Edge k of T, from P = corner k + 1 to Q = corner k + 2 (mod 3) with R = corner k, is a silhouette when topo[f, k] == -1, or the
//     named vertex R' fails the snap (w <= 0 or beyond the guard band), or the int64 orientation (X_Q - X_P)(Y_R' - Y_P) - (Y_Q - Y_P)
//     (X_R' - X_P) is not strictly opposite in sign to that of (P, Q, R): the surface folds over.  -2 is never a silhouette.
//   * A horizontal pair on row Cy = 256 py + 128 (a vertical one is the same with x and y exchanged): the edge crosses when
//     (Y_P > Cy) != (Y_Q > Cy) and tau = s (x* - Cx_N) lies in [0, 256], x* = X_P + (X_Q - X_P)(Cy - Y_P) / (Y_Q - Y_P) and s = +1 when O
//     is right of N, -1 when left; decided without dividing: with D = Y_Q - Y_P and n = s ((X_P - Cx_N) D + (X_Q - X_P)(Cy - Y_P)), both
//     negated when D < 0, as 0 <= n <= 256 D in int64.  The first edge in the order k = 0, 1, 2 that is a silhouette and crosses is used.
//   * t = ((float) n / (float) D) / 256.  t > 0.5: out[O] += (t - 0.5) (color[N] - color[O]); t < 0.5: out[N] += (0.5 - t) (color[O] -
//     color[N]).  Both vanish at t = 0.5.
//   * The forward is a gather (mesh_antialias_kernel, one lane per pixel): a pixel examines its pairs in the order left, right, up, down
//     and adds the contributions that land on it to its own colour, in that order: no atomics, bit-reproducible.  A pixel whose four
//     neighbours share its id copies its colour and leaves.
//   * The backward (mesh_antialias_backward_kernel, one lane per pixel).  g_color is a gather as well, so it is bit-reproducible: for a
//     pair that blends into pixel X with weight a = |t - 0.5| from the other pixel Y, g_color[X] -= a g_out[X] and g_color[Y] +=
//     a g_out[X]; every pixel collects both kinds from its four pairs onto g_out.  g_pos: the pixel that is the left or upper one of a
//     pair adds dL/dt = sum_c g_out[X]_c (color[N]_c - color[O]_c) times dt/d(P, Q) with float atomic adds into the zeroed g_pos
//     (not bit-reproducible): with lambda = (Cy - Y_P) / (Y_Q - Y_P) and m = (X_Q - X_P) / (Y_Q - Y_P),
//     dt/dsx_P = s (1 - lambda), dt/dsx_Q = s lambda, dt/dsy_P = -s m (1 - lambda), dt/dsy_Q = -s m lambda, then straight-through
//     to clip space as above.
#include "mesh_raster_common.h"

// dL/d(sx, sy) of vertex i, plus direct dL/dz and dL/dw, taken to clip space and added into g (one view's [V, 4])
__device__ __forceinline__ void mg_add(float* __restrict__ g, int i, const float4& p, float gsx, float gsy, float gz, float gw, int H, int W) {
  const float hx = 0.5f * (float)W, hy = 0.5f * (float)H;
  const float ax = gsx * hx, ay = gsy * hy;
  float* o = g + (int64_t)i * 4;
  atomicAdd(o + 0, ax / p.w);
  atomicAdd(o + 1, ay / p.w);
  if (gz != 0.f) atomicAdd(o + 2, gz);
  atomicAdd(o + 3, gw - (ax * (p.x / p.w) + ay * (p.y / p.w)) / p.w);
}

// ------------------------------------------------------------------------------------------------------------------ rast -> pos
__global__ void __launch_bounds__(MR_THREADS)
mesh_rasterize_backward_kernel(const float* __restrict__ pos, const int32_t* __restrict__ tri, int B, int V, int F, int H, int W,
                               const float4* __restrict__ rast, const float4* __restrict__ g_rast, float* __restrict__ g_pos) {
  const int64_t g = (int64_t)blockIdx.x * MR_THREADS + threadIdx.x;
  if (g >= (int64_t)B * H * W) return;
  const int f = (int)rast[g].w - 1;
  if (f < 0 || f >= F) return;
  const MrPixel p = mr_pixel(g, H, W);
  MrTri t;
  if (!mr_load(pos + (int64_t)p.b * V * 4, tri, f, V, H, W, 0, t)) return;
  const float4 go = g_rast[g];
  const MrPersp w = mr_persp(t, p.px, p.py);
  const float b0 = w.b0, b1 = w.b1, b2 = w.b2, q0 = w.q0, q1 = w.q1, q2 = w.q2, S = w.S;
  const float u = q0 / S, v = q1 / S;
  const float k = go.x * u + go.y * v;
  const float gq0 = (go.x - k) / S, gq1 = (go.y - k) / S, gq2 = -k / S;
  const float gb0 = gq0 / t.w0 + go.z * t.zw0, gb1 = gq1 / t.w1 + go.z * t.zw1, gb2 = gq2 / t.w2 + go.z * t.zw2;
  const float sc = 256.f * (float)t.sgn / (float)t.area;
  const float Gx = ((gb0 * (float)(t.Y1 - t.Y2) + gb1 * (float)(t.Y2 - t.Y0)) + gb2 * (float)(t.Y0 - t.Y1)) * sc;
  const float Gy = ((gb0 * (float)(t.X2 - t.X1) + gb1 * (float)(t.X0 - t.X2)) + gb2 * (float)(t.X1 - t.X0)) * sc;
  float* out = g_pos + (int64_t)p.b * V * 4;
  mg_add(out, t.i0, t.p0, -b0 * Gx, -b0 * Gy, go.z * b0 / t.w0, -(gq0 * q0 + go.z * b0 * t.zw0) / t.w0, H, W);
  mg_add(out, t.i1, t.p1, -b1 * Gx, -b1 * Gy, go.z * b1 / t.w1, -(gq1 * q1 + go.z * b1 * t.zw1) / t.w1, H, W);
  mg_add(out, t.i2, t.p2, -b2 * Gx, -b2 * Gy, go.z * b2 / t.w2, -(gq2 * q2 + go.z * b2 * t.zw2) / t.w2, H, W);
}

// ------------------------------------------------------------------------------------------------------------------ values -> rast
__global__ void __launch_bounds__(MR_THREADS)
mesh_interpolate_backward_rast_kernel(const float* __restrict__ g_out, const float* __restrict__ attr, int64_t attr_stride,
                                      const int32_t* __restrict__ idx, const float4* __restrict__ rast, int64_t pixels, int64_t per_view, int F,
                                      int N, int C, float4* __restrict__ g_rast) {
  const int64_t g = (int64_t)blockIdx.x * MR_THREADS + threadIdx.x;
  if (g >= pixels) return;
  float gu = 0.f, gv = 0.f;
  int64_t i0, i1, i2;
  if (mr_corners(rast[g], idx, F, N, i0, i1, i2)) {
    const float* a = attr + (g / per_view) * attr_stride;
    const float* go = g_out + g * C;
    for (int c = 0; c < C; c++) {
      const float a2 = a[i2 * C + c], gc = go[c];
      gu += gc * (a[i0 * C + c] - a2);
      gv += gc * (a[i1 * C + c] - a2);
    }
  }
  g_rast[g] = make_float4(gu, gv, 0.f, 0.f);
}

__global__ void __launch_bounds__(MR_THREADS)
mesh_shade_backward_rast_kernel(const float4* __restrict__ rast, const float* __restrict__ uv, const float* __restrict__ tex,
                                const float4* __restrict__ g_shaded, int64_t pixels, int F, int flip_v, int Th, int Tw,
                                float4* __restrict__ g_rast) {
  const int64_t g = (int64_t)blockIdx.x * MR_THREADS + threadIdx.x;
  if (g >= pixels) return;
  const float4 r = rast[g];
  const int f = (int)r.w - 1;
  float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
  if (f >= 0 && f < F) {
    const float4 go = g_shaded[g];
    const float gc[3] = {go.x, go.y, go.z};
    const MrShade h = mr_shade(r, uv, f, flip_v);
    const MrTap q = mr_tap(h.s, h.t, Th, Tw, 3, 0);
    float gs = 0.f, gt = 0.f;
#pragma unroll
    for (int c = 0; c < 3; c++) mr_tap_slopes(q, tex, c, gc[c], gs, gt);
    gs *= (float)Tw;
    gt *= (float)Th;      // the gradient to the interpolated t, which is built from the flipped v
    out.x = gs * (h.a[0] - h.a[4]) + gt * (h.v0 - h.v2);
    out.y = gs * (h.a[2] - h.a[4]) + gt * (h.v1 - h.v2);
  }
  g_rast[g] = out;
}

// ------------------------------------------------------------------------------------------------------------------ antialias
struct MgHit {
  int n_is_a;        // the near pixel is the pair's first (left or upper) pixel
  int to_a;          // the blend lands on the pair's first pixel
  float alpha;       // |t - 0.5|, 0: nothing to blend
  int iP, iQ;        // the edge's vertices
  float lam, m, s;   // lambda, m and s of the header
};

// One edge of T against the pair: (aP, cP), (aQ, cQ), (aR, cR) are the corners' coordinates along and across the pair's axis, Cn the near
// pixel's centre along the axis, Cr the centre across it.  true: the edge is a silhouette and crosses; t, lam, m are set.
__device__ __forceinline__ bool mg_edge(const float* __restrict__ view, int V, int H, int W, int axis, int nb, int aP, int cP, int aQ, int cQ,
                                        int aR, int cR, int Cn, int Cr, int s, float& t, float& lam, float& m) {
  if ((cP > Cr) == (cQ > Cr)) return false;
  int64_t D = (int64_t)cQ - cP;
  int64_t n = s * ((int64_t)(aP - Cn) * D + (int64_t)(aQ - aP) * (Cr - cP));
  if (D < 0) {
    D = -D;
    n = -n;
  }
  if (n < 0 || n > 256 * D) return false;
  if (nb != -1) {
    if (nb < 0 || nb >= V) return false;      // -2, or no vertex: never a silhouette
    const float4 p = ((const float4*)view)[nb];
    int X, Y;
    if (p.w > 0.f && mr_snap(p.x, p.w, W, X) && mr_snap(p.y, p.w, H, Y)) {
      const int a2 = axis ? Y : X, c2 = axis ? X : Y;
      // the orientation's sign changes with the exchange of the axes for both triples alike
      const int64_t o = (int64_t)(aQ - aP) * (cR - cP) - (int64_t)(cQ - cP) * (aR - aP);
      const int64_t o2 = (int64_t)(aQ - aP) * (c2 - cP) - (int64_t)(cQ - cP) * (a2 - aP);
      if ((o > 0 && o2 < 0) || (o < 0 && o2 > 0)) return false;
    }
  }
  t = ((float)n / (float)D) / 256.f;
  lam = (float)(Cr - cP) / (float)(cQ - cP);
  m = (float)(aQ - aP) / (float)(cQ - cP);
  return true;
}

// The pair of pixel a = (ax, ay) and pixel b = a + (1, 0) (axis 0) or a + (0, 1) (axis 1), ra and rb their rast.  h.alpha == 0 when
// nothing blends.
__device__ __forceinline__ void mg_pair(const float* __restrict__ view, const int32_t* __restrict__ tri, const int32_t* __restrict__ topo, int V,
                                        int F, int H, int W, const float4& ra, const float4& rb, int ax, int ay, int axis, MgHit& h) {
  h.alpha = 0.f;
  const int ida = (int)ra.w, idb = (int)rb.w;
  if (ida == idb) return;
  const bool n_is_a = ida > 0 && (!(idb > 0) || ra.z < rb.z || (ra.z == rb.z && ida < idb));
  const int f = (n_is_a ? ida : idb) - 1;
  if (f < 0 || f >= F) return;
  MrTri T;
  if (!mr_load(view, tri, f, V, H, W, 0, T)) return;
  const int s = n_is_a ? 1 : -1;
  // along / across the pair's axis
  const int A0 = axis ? T.Y0 : T.X0, C0 = axis ? T.X0 : T.Y0, A1 = axis ? T.Y1 : T.X1, C1 = axis ? T.X1 : T.Y1, A2 = axis ? T.Y2 : T.X2,
            C2 = axis ? T.X2 : T.Y2;
  const int na = (axis ? ay : ax) + (n_is_a ? 0 : 1), cr = axis ? ax : ay;
  const int Cn = 256 * na + 128, Cr = 256 * cr + 128;
  const int32_t* nb = topo + (int64_t)f * 3;
  float t, lam, m;
  if (mg_edge(view, V, H, W, axis, nb[0], A1, C1, A2, C2, A0, C0, Cn, Cr, s, t, lam, m)) {
    h.iP = T.i1;
    h.iQ = T.i2;
  } else if (mg_edge(view, V, H, W, axis, nb[1], A2, C2, A0, C0, A1, C1, Cn, Cr, s, t, lam, m)) {
    h.iP = T.i2;
    h.iQ = T.i0;
  } else if (mg_edge(view, V, H, W, axis, nb[2], A0, C0, A1, C1, A2, C2, Cn, Cr, s, t, lam, m)) {
    h.iP = T.i0;
    h.iQ = T.i1;
  } else {
    return;
  }
  h.n_is_a = n_is_a;
  h.lam = lam;
  h.m = m;
  h.s = (float)s;
  if (t > 0.5f) {
    h.alpha = t - 0.5f;
    h.to_a = !n_is_a;
  } else if (t < 0.5f) {
    h.alpha = 0.5f - t;
    h.to_a = n_is_a;
  }
}

// The four pairs of pixel g = (px, py) of a view in the order left, right, up, down: other[k] is the other pixel's index (g itself where
// there is none), mine[k] says that the pair's blend lands here.  false: all four neighbours share the pixel's id.
__device__ __forceinline__ bool mg_pairs(const float* __restrict__ view, const int32_t* __restrict__ tri, const int32_t* __restrict__ topo,
                                         const float4* __restrict__ rast, int64_t g, int px, int py, int V, int F, int H, int W, MgHit h[4],
                                         int64_t other[4], bool mine[4]) {
  const float4 r = rast[g];
  other[0] = px > 0 ? g - 1 : g;
  other[1] = px < W - 1 ? g + 1 : g;
  other[2] = py > 0 ? g - W : g;
  other[3] = py < H - 1 ? g + W : g;
  const float4 r0 = rast[other[0]], r1 = rast[other[1]], r2 = rast[other[2]], r3 = rast[other[3]];
  if (r0.w == r.w && r1.w == r.w && r2.w == r.w && r3.w == r.w) return false;
  mg_pair(view, tri, topo, V, F, H, W, r0, r, px - 1, py, 0, h[0]);
  mg_pair(view, tri, topo, V, F, H, W, r, r1, px, py, 0, h[1]);
  mg_pair(view, tri, topo, V, F, H, W, r2, r, px, py - 1, 1, h[2]);
  mg_pair(view, tri, topo, V, F, H, W, r, r3, px, py, 1, h[3]);
  mine[0] = h[0].alpha != 0.f && !h[0].to_a;
  mine[1] = h[1].alpha != 0.f && h[1].to_a;
  mine[2] = h[2].alpha != 0.f && !h[2].to_a;
  mine[3] = h[3].alpha != 0.f && h[3].to_a;
  return true;
}

__global__ void __launch_bounds__(MR_THREADS)
mesh_antialias_kernel(const float* __restrict__ color, int C, const float4* __restrict__ rast, const float* __restrict__ pos,
                      const int32_t* __restrict__ tri, const int32_t* __restrict__ topo, int B, int V, int F, int H, int W,
                      float* __restrict__ out) {
  const int64_t g = (int64_t)blockIdx.x * MR_THREADS + threadIdx.x;
  if (g >= (int64_t)B * H * W) return;
  const MrPixel p = mr_pixel(g, H, W);
  MgHit h[4];
  int64_t other[4];
  bool mine[4];
  const float* cx = color + g * C;
  float* o = out + g * C;
  if (!mg_pairs(pos + (int64_t)p.b * V * 4, tri, topo, rast, g, p.px, p.py, V, F, H, W, h, other, mine)) {
    for (int c = 0; c < C; c++) o[c] = cx[c];
    return;
  }
  for (int c = 0; c < C; c++) {
    const float own = cx[c];
    float v = own;
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (mine[k]) v += h[k].alpha * (color[other[k] * C + c] - own);
    o[c] = v;
  }
}

__global__ void __launch_bounds__(MR_THREADS)
mesh_antialias_backward_kernel(const float* __restrict__ color, int C, const float4* __restrict__ rast, const float* __restrict__ pos,
                               const int32_t* __restrict__ tri, const int32_t* __restrict__ topo, int B, int V, int F, int H, int W,
                               const float* __restrict__ g_out, float* __restrict__ g_color, float* __restrict__ g_pos) {
  const int64_t g = (int64_t)blockIdx.x * MR_THREADS + threadIdx.x;
  if (g >= (int64_t)B * H * W) return;
  const MrPixel p = mr_pixel(g, H, W);
  MgHit h[4];
  int64_t other[4];
  bool mine[4];
  const float* view = pos + (int64_t)p.b * V * 4;
  const float* go = g_out + g * C;
  if (!mg_pairs(view, tri, topo, rast, g, p.px, p.py, V, F, H, W, h, other, mine)) {
    if (g_color)
      for (int c = 0; c < C; c++) g_color[g * C + c] = go[c];
    return;
  }
  if (g_color) {
    for (int c = 0; c < C; c++) {
      const float own = go[c];
      float v = own;
#pragma unroll
      for (int k = 0; k < 4; k++)
        if (h[k].alpha != 0.f) v += mine[k] ? -(h[k].alpha * own) : h[k].alpha * g_out[other[k] * C + c];
      g_color[g * C + c] = v;
    }
  }
  if (!g_pos) return;
  float* gp = g_pos + (int64_t)p.b * V * 4;
#pragma unroll
  for (int k = 1; k < 4; k += 2) {      // the pairs in which this pixel is the first: right, down
    if (h[k].alpha == 0.f) continue;
    const int64_t pa = g, pb = other[k];
    const int64_t pn = h[k].n_is_a ? pa : pb, po = h[k].n_is_a ? pb : pa, pt = h[k].to_a ? pa : pb;
    float dt = 0.f;
    for (int c = 0; c < C; c++) dt += g_out[pt * C + c] * (color[pn * C + c] - color[po * C + c]);
    const float s = h[k].s, lam = h[k].lam, m = h[k].m;
    const float along_p = dt * s * (1.f - lam), along_q = dt * s * lam;
    const float across_p = -(along_p * m), across_q = -(along_q * m);
    const float4 pP = ((const float4*)view)[h[k].iP], pQ = ((const float4*)view)[h[k].iQ];
    if (k == 1) {      // a horizontal pair: along is x
      mg_add(gp, h[k].iP, pP, along_p, across_p, 0.f, 0.f, H, W);
      mg_add(gp, h[k].iQ, pQ, along_q, across_q, 0.f, 0.f, H, W);
    } else {
      mg_add(gp, h[k].iP, pP, across_p, along_p, 0.f, 0.f, H, W);
      mg_add(gp, h[k].iQ, pQ, across_q, along_q, 0.f, 0.f, H, W);
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------ C-ABI
extern "C" int gip_mesh_rasterize_backward(const float* pos, const int32_t* tri, int32_t B, int64_t V, int64_t F, int32_t H, int32_t W,
                                           const float* rast, const float* g_rast, float* g_pos, void* stream) {
  if (!mr_mesh_ok(B, V, F, H, W) || !rast || !g_rast) return 1;
  if (F == 0 || V == 0) return 0;
  if (!pos || !tri || !g_pos) return 1;
  const int64_t pixels = (int64_t)B * H * W;
  hipLaunchKernelGGL(mesh_rasterize_backward_kernel, dim3(mesh_blocks(pixels)), dim3(MR_THREADS), 0, (hipStream_t)stream, pos, tri, (int)B,
                     (int)V, (int)F, (int)H, (int)W, (const float4*)rast, (const float4*)g_rast, g_pos);
  return mesh_done();
}

extern "C" int gip_mesh_interpolate_backward_rast(const float* g_out, const float* attr, int32_t attr_batch, int64_t N, int32_t C,
                                                  const int32_t* idx, int64_t F, const float* rast, int32_t B, int32_t H, int32_t W,
                                                  float* g_rast, void* stream) {
  if (!mr_attr_ok(attr, attr_batch, N, C, idx, F, B, H, W) || !rast || !g_out || !g_rast) return 1;
  const int64_t pixels = (int64_t)B * H * W;
  hipLaunchKernelGGL(mesh_interpolate_backward_rast_kernel, dim3(mesh_blocks(pixels)), dim3(MR_THREADS), 0, (hipStream_t)stream, g_out, attr,
                     mr_stride(attr_batch, N * C), idx, (const float4*)rast, pixels, (int64_t)H * W, (int)F, (int)N, (int)C,
                     (float4*)g_rast);
  return mesh_done();
}

extern "C" int gip_mesh_shade_backward_rast(const float* rast, const float* uv, int64_t F, int32_t flip_v, const float* tex, int32_t Th,
                                            int32_t Tw, const float* g_shaded, int32_t B, int32_t H, int32_t W, float* g_rast, void* stream) {
  if (!mr_image_ok(B, H, W) || !mr_tex_ok(Th, Tw, 3) || F < 0 || F > MR_MAX_FACES || !rast || !tex || !g_shaded || !g_rast) return 1;
  if (F > 0 && !uv) return 1;
  const int64_t pixels = (int64_t)B * H * W;
  hipLaunchKernelGGL(mesh_shade_backward_rast_kernel, dim3(mesh_blocks(pixels)), dim3(MR_THREADS), 0, (hipStream_t)stream, (const float4*)rast,
                     uv, tex, (const float4*)g_shaded, pixels, (int)F, (int)(flip_v != 0), (int)Th, (int)Tw, (float4*)g_rast);
  return mesh_done();
}

static int mg_antialias_ok(const float* color, int32_t C, const float* rast, const float* pos, const int32_t* tri, const int32_t* topo,
                           int32_t B, int64_t V, int64_t F, int32_t H, int32_t W) {
  if (!mr_mesh_ok(B, V, F, H, W) || C < 1 || (int64_t)B * H * W * C > INT32_MAX || !color || !rast) return 0;
  return F == 0 || V == 0 || (pos && tri && topo);
}

extern "C" int gip_mesh_antialias(const float* color, int32_t C, const float* rast, const float* pos, const int32_t* tri, const int32_t* topo,
                                  int32_t B, int64_t V, int64_t F, int32_t H, int32_t W, float* out, void* stream) {
  if (!mg_antialias_ok(color, C, rast, pos, tri, topo, B, V, F, H, W) || !out) return 1;
  const int64_t pixels = (int64_t)B * H * W;
  hipLaunchKernelGGL(mesh_antialias_kernel, dim3(mesh_blocks(pixels)), dim3(MR_THREADS), 0, (hipStream_t)stream, color, (int)C,
                     (const float4*)rast, pos, tri, topo, (int)B, (int)V, (int)F, (int)H, (int)W, out);
  return mesh_done();
}

extern "C" int gip_mesh_antialias_backward(const float* color, int32_t C, const float* rast, const float* pos, const int32_t* tri,
                                           const int32_t* topo, int32_t B, int64_t V, int64_t F, int32_t H, int32_t W, const float* g_out,
                                           float* g_color, float* g_pos, void* stream) {
  if (!mg_antialias_ok(color, C, rast, pos, tri, topo, B, V, F, H, W) || !g_out) return 1;
  if (!g_color && !g_pos) return 0;
  const int64_t pixels = (int64_t)B * H * W;
  hipLaunchKernelGGL(mesh_antialias_backward_kernel, dim3(mesh_blocks(pixels)), dim3(MR_THREADS), 0, (hipStream_t)stream, color, (int)C,
                     (const float4*)rast, pos, tri, topo, (int)B, (int)V, (int)F, (int)H, (int)W, g_out, g_color, g_pos);
  return mesh_done();
}
