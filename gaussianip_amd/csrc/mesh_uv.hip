// mesh_uv.hip — unwrapping a triangle mesh into a chart atlas, the tangents that need its UVs and the padding of a baked texture's
// seams (gaussianip_amd/utils/uv_atlas.py; DESIGN.md "Unwrapping the mesh").  In place of the reference's xatlas unwrapping
// (threestudio/models/mesh.py:207-250), Mesh._compute_vertex_tangent (mesh.py:162-205) and the exporter's cv2.inpaint
// (threestudio/models/exporters/mesh_exporter.py:53-137).  Linked into libgip_model.so, built with -ffp-contract=off: every float
// operation below is one correctly rounded float32 operation in the order written, which tests/uv_atlas_reference.py restates.
// No kernel here spins or waits on another workgroup; every loop over rounds lives on the host.
//
// Charts.  face_nbr [F, 3] (the face across edge (k, k + 1 mod 3), -1 without exactly one opposite partner) is the host's table.
//   normals   n_f = cross(p1 - p0, p2 - p0), not normalised; 0 for a face with an index outside [0, V).
//   smooth    one round: m'_f = ((m_f + m_nbr0) + m_nbr1) + m_nbr2, a missing neighbour skipped; ping-pong, a gather.
//   classes   class(v) = 2 axis + (v[axis] < 0), axis the first of x, y, z with the largest |component|.  A face takes class(m_f) when
//             n_f . d >= min_cos sqrtf(n_f . n_f) for that class's direction d (n_f . d is plus or minus one component of n_f), else
//             class(n_f); class 4 when n_f . n_f <= 1e-20.
//   labels    min-label propagation with pointer jumping over the face graph, an edge being a face_nbr entry between two faces of one
//             class: uv_hook_kernel / uv_compress_kernel, the scheme of mesh_common.h "Labels" (which proves that the fixed point is the
//             component's smallest index whatever the interleaving).  label[f] starts as f.
// Rectangles.  A chart's class gives its projection: +x (y, z), -x (z, y), +y (z, x), -y (x, z), +z (x, y), -z (y, x), so that a face
//   whose normal points along the class direction is counter-clockwise in (u, v).  uv_box_kernel takes the minimum and maximum of (u, v)
//   over the corners of a chart's faces with integer atomics on mesh_common.h's float key.  The caller initialises the keys (minima
//   0xffffffff, maxima 0) and decodes them.
// Texture vertices.  uv_place_kernel, one lane per texture vertex (a distinct (chart, vertex) pair): with the chart's row
//   (umin, vmin, ox, oy) — ox = x0 + pad, oy = y0 + pad as floats — and the atlas' scale s,
//       x = ox + (u - umin) * s      y = oy + (v - vmin) * s      vt = ((x + 0.5) / T, 1 - (y + 0.5) / T)
//   x, y are texel-index coordinates (a texel's centre is an integer, row 0 on top); vt is the OBJ convention of utils.texture.atlas_uv.
// Tangents.  Per face (tang_f, kept for the backward), with e1 = p1 - p0, e2 = p2 - p0, a = t1 - t0, b = t2 - t0 of its texture vertices:
//       tang = (e1 * b.y - e2 * a.y) / den      den = a.x b.y - a.y b.x, clamped away from 0 to +-1e-6 (den > 0 ? max : min)
//   per vertex, a gather over its corners in corner_list order: mean = sum / count, t1 = mean / max(|mean|, 1e-12),
//   t2 = t1 - (t1 . n) n, out = t2 / max(|t2|, 1e-12).  A vertex without a corner gets (1, 0, 0) and sends no gradient (the reference
//   divides 0 by 0 there).  The backward: uv_tangent_vertex_backward_kernel recomputes the vertex's chain and writes g_n and
//   g_sum = dL/dsum; uv_tangent_face_backward_kernel turns g_sum[i0] + g_sum[i1] + g_sum[i2] into the face's (g_e1, g_e2);
//   uv_tangent_gather_backward_kernel adds per vertex over its corners: corner 1 takes g_e1, corner 2 g_e2, corner 0 minus their sum.
//   Gathers only, one lane per vertex or face in table order: no float atomics, bitwise equal from run to run.  UVs are constants.
// Dilation.  uv_dilate_kernel, one lane per texel and round: a filled texel is copied; an unfilled one with k >= 1 filled 8-neighbours
//   (as filled BEFORE the round) becomes their sum in row-major neighbour order divided by (float) k and is filled after the round;
//   any other texel is written as 0 and stays unfilled.  The host ping-pongs two buffers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gip_model.h"
#include "mesh_common.h"

// ---------------------------------------------------------------------------------------------------------------------- charts
__global__ void __launch_bounds__(MESH_THREADS)
uv_face_normals_kernel(const float* __restrict__ pos, const int32_t* __restrict__ faces, int64_t V, int64_t F, float* __restrict__ normals) {
  const int64_t f = (int64_t)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (f < F) mesh_store(normals, f, mesh_face_cross(pos, faces, f, V));
}

__global__ void __launch_bounds__(MESH_THREADS)
uv_smooth_kernel(const float* __restrict__ src, const int32_t* __restrict__ face_nbr, int64_t F, float* __restrict__ dst) {
  const int64_t f = (int64_t)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (f >= F) return;
  MeshVec m = mesh_load(src, f);
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const int64_t g = face_nbr[3 * f + k];
    if ((uint64_t)g < (uint64_t)F) m = mesh_add(m, mesh_load(src, g));
  }
  mesh_store(dst, f, m);
}

__device__ __forceinline__ int uv_class_of(MeshVec v) {
  int axis = 0;
  float best = fabsf(v.x);
  if (fabsf(v.y) > best) { axis = 1; best = fabsf(v.y); }
  if (fabsf(v.z) > best) axis = 2;
  return 2 * axis + (mesh_comp(v, axis) < 0.f ? 1 : 0);
}

__global__ void __launch_bounds__(MESH_THREADS)
uv_class_kernel(const float* __restrict__ normals, const float* __restrict__ smoothed, int64_t F, float min_cos,
                int32_t* __restrict__ face_class) {
  const int64_t f = (int64_t)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (f >= F) return;
  const MeshVec n = mesh_load(normals, f);
  const float d = mesh_dot(n, n);
  int cls = 4;
  if (d > 1e-20f) {
    cls = uv_class_of(mesh_load(smoothed, f));
    const float along = mesh_comp(n, cls >> 1);
    const float nd = (cls & 1) ? -along : along;
    if (!(nd >= min_cos * sqrtf(d))) cls = uv_class_of(n);
  }
  face_class[f] = cls;
}

__global__ void __launch_bounds__(MESH_THREADS)
uv_hook_kernel(const int32_t* __restrict__ face_nbr, const int32_t* __restrict__ face_class, int F, int32_t* label,
               int32_t* __restrict__ changed) {
  const int f = blockIdx.x * MESH_THREADS + threadIdx.x;
  if (f >= F) return;
  const int cls = face_class[f];
  bool moved = false;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const int g = face_nbr[(int64_t)f * 3 + k];
    if (g < 0 || g >= F || face_class[g] != cls) continue;
    // relaxed reads: other lanes lower these words meanwhile; any value seen is a label in [0, F) of this component
    const int lf = __atomic_load_n(label + f, __ATOMIC_RELAXED), lg = __atomic_load_n(label + g, __ATOMIC_RELAXED);
    if (lf == lg) continue;
    const int m = min(lf, lg), big = max(lf, lg), owner = lf > lg ? f : g;
    if (atomicMin(label + big, m) > m) moved = true;      // big in [0, F): it was read from label
    if (atomicMin(label + owner, m) > m) moved = true;
  }
  if (moved) *changed = 1;
}

__global__ void __launch_bounds__(MESH_THREADS)
uv_compress_kernel(int F, int32_t* label, int32_t* __restrict__ changed) {
  mesh_label_compress(label, blockIdx.x * MESH_THREADS + threadIdx.x, F, changed);
}

// ------------------------------------------------------------------------------------------------------------------ rectangles
// the two kept coordinates of p under class cls, counter-clockwise for a face that looks along the class direction
__device__ __forceinline__ void uv_project(MeshVec p, int cls, float* u, float* v) {
  switch (cls) {
    case 0: *u = p.y; *v = p.z; break;
    case 1: *u = p.z; *v = p.y; break;
    case 2: *u = p.z; *v = p.x; break;
    case 3: *u = p.x; *v = p.z; break;
    case 4: *u = p.x; *v = p.y; break;
    default: *u = p.y; *v = p.x; break;
  }
}

__global__ void __launch_bounds__(MESH_THREADS)
uv_box_kernel(const float* __restrict__ pos, const int32_t* __restrict__ faces, const int32_t* __restrict__ face_chart,
              const int32_t* __restrict__ chart_class, int64_t V, int64_t F, int64_t C, uint32_t* __restrict__ box) {
  const int64_t f = (int64_t)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (f >= F) return;
  int32_t idx[3];
  if (!mesh_face(faces, f, V, &idx[0], &idx[1], &idx[2])) return;
  const int64_t c = face_chart[f];
  if ((uint64_t)c >= (uint64_t)C) return;      // not a chart of this atlas: nothing is written outside the table
  const int cls = chart_class[c];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    float u, v;
    uv_project(mesh_load(pos, idx[k]), cls, &u, &v);
    const uint32_t ku = mesh_float_key(u), kv = mesh_float_key(v);
    atomicMin(box + 4 * c, ku);
    atomicMin(box + 4 * c + 1, kv);
    atomicMax(box + 4 * c + 2, ku);
    atomicMax(box + 4 * c + 3, kv);
  }
}

__global__ void __launch_bounds__(MESH_THREADS)
uv_place_kernel(const float* __restrict__ pos, const int32_t* __restrict__ vmapping, const int32_t* __restrict__ vt_chart,
                const int32_t* __restrict__ chart_class, const float* __restrict__ chart_origin, int64_t V, int64_t Vt, int64_t C,
                float scale, float size, float* __restrict__ v_tex) {
  const int64_t t = (int64_t)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (t >= Vt) return;
  const int64_t p = vmapping[t], c = vt_chart[t];
  float x = 0.f, y = 0.f;
  if ((uint64_t)p < (uint64_t)V && (uint64_t)c < (uint64_t)C) {
    float u, v;
    uv_project(mesh_load(pos, p), chart_class[c], &u, &v);
    x = chart_origin[4 * c + 2] + (u - chart_origin[4 * c]) * scale;
    y = chart_origin[4 * c + 3] + (v - chart_origin[4 * c + 1]) * scale;
  }
  v_tex[2 * t] = (x + 0.5f) / size;
  v_tex[2 * t + 1] = 1.f - (y + 0.5f) / size;
}

// -------------------------------------------------------------------------------------------------------------------- tangents
// the face's clamped denominator and the two uv factors of its numerator; false when an index lies outside its table
__device__ __forceinline__ bool uv_tangent_face(const int32_t* __restrict__ tex_idx, const float* __restrict__ v_tex, int64_t f, int64_t Vt,
                                                float* ay, float* by, float* den) {
  const int64_t t0 = tex_idx[3 * f], t1 = tex_idx[3 * f + 1], t2 = tex_idx[3 * f + 2];
  if ((uint64_t)t0 >= (uint64_t)Vt || (uint64_t)t1 >= (uint64_t)Vt || (uint64_t)t2 >= (uint64_t)Vt) return false;
  const float ax = v_tex[2 * t1] - v_tex[2 * t0], bx = v_tex[2 * t2] - v_tex[2 * t0];
  *ay = v_tex[2 * t1 + 1] - v_tex[2 * t0 + 1];
  *by = v_tex[2 * t2 + 1] - v_tex[2 * t0 + 1];
  const float d = ax * *by - *ay * bx;
  *den = d > 0.f ? fmaxf(d, 1e-6f) : fminf(d, -1e-6f);
  return true;
}

__global__ void __launch_bounds__(MESH_THREADS)
uv_tangent_face_kernel(const float* __restrict__ pos, const int32_t* __restrict__ faces, const int32_t* __restrict__ tex_idx,
                       const float* __restrict__ v_tex, int64_t V, int64_t F, int64_t Vt, float* __restrict__ tang) {
  const int64_t f = (int64_t)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (f >= F) return;
  int32_t i0, i1, i2;
  float ay, by, den;
  MeshVec t = MeshVec{0.f, 0.f, 0.f};
  if (mesh_face(faces, f, V, &i0, &i1, &i2) && uv_tangent_face(tex_idx, v_tex, f, Vt, &ay, &by, &den)) {
    const MeshVec p0 = mesh_load(pos, i0);
    const MeshVec e1 = mesh_sub(mesh_load(pos, i1), p0), e2 = mesh_sub(mesh_load(pos, i2), p0);
    t = mesh_div(mesh_sub(mesh_scale(e1, by), mesh_scale(e2, ay)), den);
  }
  mesh_store(tang, f, t);
}

// the vertex's chain up to the output; count == 0: no corner
struct UvTangent { MeshVec t1, out; float q1, q2, l1, l2, dn, count; };

__device__ __forceinline__ UvTangent uv_tangent_vertex(const int32_t* __restrict__ corner_start, const int32_t* __restrict__ corner_list,
                                                       const float* __restrict__ tang, const float* __restrict__ nrm, int64_t v, int64_t F) {
  int64_t lo, hi;
  mesh_row(corner_start, v, 3 * F, &lo, &hi);
  MeshVec s = MeshVec{0.f, 0.f, 0.f};
  float count = 0.f;
  for (int64_t at = lo; at < hi; at++) {
    const int64_t c = corner_list[at];
    if ((uint64_t)c >= (uint64_t)(3 * F)) continue;
    s = mesh_add(s, mesh_load(tang, c / 3));
    count += 1.f;
  }
  UvTangent r;
  r.count = count;
  if (count == 0.f) {
    r.t1 = r.out = MeshVec{1.f, 0.f, 0.f};
    r.q1 = r.q2 = r.l1 = r.l2 = 1.f;
    r.dn = 0.f;
    return r;
  }
  const MeshVec mean = mesh_div(s, count);
  r.l1 = sqrtf(mesh_dot(mean, mean));
  r.q1 = fmaxf(r.l1, 1e-12f);
  r.t1 = mesh_div(mean, r.q1);
  const MeshVec n = mesh_load(nrm, v);
  r.dn = mesh_dot(r.t1, n);
  const MeshVec t2 = mesh_sub(r.t1, mesh_scale(n, r.dn));
  r.l2 = sqrtf(mesh_dot(t2, t2));
  r.q2 = fmaxf(r.l2, 1e-12f);
  r.out = mesh_div(t2, r.q2);
  return r;
}

__global__ void __launch_bounds__(MESH_THREADS)
uv_tangent_vertex_kernel(const int32_t* __restrict__ corner_start, const int32_t* __restrict__ corner_list, const float* __restrict__ tang,
                         const float* __restrict__ nrm, int64_t V, int64_t F, float* __restrict__ out) {
  const int64_t v = (int64_t)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (v >= V) return;
  mesh_store(out, v, uv_tangent_vertex(corner_start, corner_list, tang, nrm, v, F).out);
}

// x / max(|x|, eps) differentiated as autograd does: g / q, minus y (y . g) / q where the length was not clamped
__device__ __forceinline__ MeshVec uv_normalize_backward(MeshVec y, float l, float q, MeshVec g) {
  MeshVec r = mesh_div(g, q);
  if (l > 1e-12f) r = mesh_sub(r, mesh_div(mesh_scale(y, mesh_dot(y, g)), q));
  return r;
}

__global__ void __launch_bounds__(MESH_THREADS)
uv_tangent_vertex_backward_kernel(const int32_t* __restrict__ corner_start, const int32_t* __restrict__ corner_list,
                                  const float* __restrict__ tang, const float* __restrict__ nrm, const float* __restrict__ g_out, int64_t V,
                                  int64_t F, float* __restrict__ g_sum, float* __restrict__ g_nrm) {
  const int64_t v = (int64_t)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (v >= V) return;
  const UvTangent r = uv_tangent_vertex(corner_start, corner_list, tang, nrm, v, F);
  MeshVec gs = MeshVec{0.f, 0.f, 0.f}, gn = MeshVec{0.f, 0.f, 0.f};
  if (r.count > 0.f) {
    const MeshVec n = mesh_load(nrm, v);
    const MeshVec g2 = uv_normalize_backward(r.out, r.l2, r.q2, mesh_load(g_out, v));      // to t2 = t1 - (t1 . n) n
    const float gd = mesh_dot(g2, n);
    const MeshVec g1 = mesh_sub(g2, mesh_scale(n, gd));
    gn = mesh_neg(mesh_add(mesh_scale(r.t1, gd), mesh_scale(g2, r.dn)));
    gs = mesh_div(uv_normalize_backward(r.t1, r.l1, r.q1, g1), r.count);
  }
  mesh_store(g_sum, v, gs);
  mesh_store(g_nrm, v, gn);
}

__global__ void __launch_bounds__(MESH_THREADS)
uv_tangent_face_backward_kernel(const int32_t* __restrict__ faces, const int32_t* __restrict__ tex_idx, const float* __restrict__ v_tex,
                                const float* __restrict__ g_sum, int64_t V, int64_t F, int64_t Vt, float* __restrict__ g_edge) {
  const int64_t f = (int64_t)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (f >= F) return;
  int32_t i0, i1, i2;
  float ay, by, den;
  MeshVec g1 = MeshVec{0.f, 0.f, 0.f}, g2 = g1;
  if (mesh_face(faces, f, V, &i0, &i1, &i2) && uv_tangent_face(tex_idx, v_tex, f, Vt, &ay, &by, &den)) {
    const MeshVec g = mesh_div(mesh_add(mesh_add(mesh_load(g_sum, i0), mesh_load(g_sum, i1)), mesh_load(g_sum, i2)), den);
    g1 = mesh_scale(g, by);
    g2 = mesh_scale(g, -ay);
  }
  mesh_store(g_edge, 2 * f, g1);
  mesh_store(g_edge, 2 * f + 1, g2);
}

__global__ void __launch_bounds__(MESH_THREADS)
uv_tangent_gather_backward_kernel(const int32_t* __restrict__ corner_start, const int32_t* __restrict__ corner_list,
                                  const float* __restrict__ g_edge, int64_t V, int64_t F, float* __restrict__ g_pos) {
  const int64_t v = (int64_t)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (v >= V) return;
  int64_t lo, hi;
  mesh_row(corner_start, v, 3 * F, &lo, &hi);
  MeshVec acc = MeshVec{0.f, 0.f, 0.f};
  for (int64_t at = lo; at < hi; at++) {
    const int64_t c = corner_list[at];
    if ((uint64_t)c >= (uint64_t)(3 * F)) continue;
    const int64_t f = c / 3;
    acc = mesh_add(acc, mesh_corner_share((int)(c - 3 * f), mesh_load(g_edge, 2 * f), mesh_load(g_edge, 2 * f + 1)));
  }
  mesh_store(g_pos, v, acc);
}

// -------------------------------------------------------------------------------------------------------------------- dilation
__global__ void __launch_bounds__(MESH_THREADS)
uv_dilate_kernel(const float* __restrict__ src, const uint8_t* __restrict__ src_mask, int H, int W, int C, float* __restrict__ dst,
                 uint8_t* __restrict__ dst_mask) {
  const int64_t at = (int64_t)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (at >= (int64_t)H * W) return;
  const int y = (int)(at / W), x = (int)(at - (int64_t)y * W);
  if (src_mask[at]) {
    for (int c = 0; c < C; c++) dst[at * C + c] = src[at * C + c];
    dst_mask[at] = 1;
    return;
  }
  int count = 0;
  for (int dy = -1; dy <= 1; dy++)
    for (int dx = -1; dx <= 1; dx++) {
      const int yy = y + dy, xx = x + dx;
      if ((dy | dx) != 0 && yy >= 0 && yy < H && xx >= 0 && xx < W && src_mask[(int64_t)yy * W + xx]) count++;
    }
  for (int c = 0; c < C; c++) {
    float sum = 0.f;
    for (int dy = -1; dy <= 1; dy++)
      for (int dx = -1; dx <= 1; dx++) {
        const int yy = y + dy, xx = x + dx;
        if ((dy | dx) != 0 && yy >= 0 && yy < H && xx >= 0 && xx < W && src_mask[(int64_t)yy * W + xx])
          sum += src[((int64_t)yy * W + xx) * C + c];
      }
    dst[at * C + c] = count ? sum / (float)count : 0.f;
  }
  dst_mask[at] = count ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------------------------------ host
extern "C" int gip_uv_face_classes(const float* pos, const int32_t* faces, const int32_t* face_nbr, int64_t V, int64_t F,
                                   int32_t smooth_rounds, float min_cos, float* normals, float* smooth_a, float* smooth_b,
                                   int32_t* face_class, void* stream) {
  if (!mesh_sizes_ok(V, F) || smooth_rounds < 0 || smooth_rounds > 64 || !(min_cos >= 0.f) || !(min_cos <= 0.5f)) return 1;
  if (F == 0) return 0;
  if (!pos || !faces || !face_nbr || !normals || !face_class || (smooth_rounds > 0 && (!smooth_a || !smooth_b))) return 1;
  const int64_t blocks = mesh_blocks(F);
  MESH_LAUNCH(uv_face_normals_kernel, blocks, stream, pos, faces, V, F, normals);
  const float* cur = normals;
  for (int r = 0; r < smooth_rounds; r++) {
    float* dst = (r & 1) ? smooth_b : smooth_a;
    MESH_LAUNCH(uv_smooth_kernel, blocks, stream, cur, face_nbr, F, dst);
    cur = dst;
  }
  MESH_LAUNCH(uv_class_kernel, blocks, stream, (const float*)normals, cur, F, min_cos, face_class);
  return mesh_done();
}

extern "C" int gip_uv_chart_rounds(const int32_t* face_nbr, const int32_t* face_class, int64_t F, int32_t* labels, int32_t* changed,
                                   int32_t rounds, void* stream) {
  if (F < 0 || F > INT32_MAX / 3 || rounds < 1 || rounds > 64) return 1;
  if (F == 0) return 0;
  if (!face_nbr || !face_class || !labels || !changed) return 1;
  const int64_t blocks = mesh_blocks(F);
  for (int r = 0; r < rounds; r++) {
    MESH_LAUNCH(uv_hook_kernel, blocks, stream, face_nbr, face_class, (int)F, labels, changed);
    MESH_LAUNCH(uv_compress_kernel, blocks, stream, (int)F, labels, changed);
  }
  return mesh_done();
}

extern "C" int gip_uv_chart_boxes(const float* pos, const int32_t* faces, const int32_t* face_chart, const int32_t* chart_class, int64_t V,
                                  int64_t F, int64_t C, uint32_t* box_keys, void* stream) {
  if (!mesh_sizes_ok(V, F) || C < 0 || C > F) return 1;
  if (F == 0 || C == 0) return 0;
  if (!pos || !faces || !face_chart || !chart_class || !box_keys) return 1;
  MESH_LAUNCH(uv_box_kernel, mesh_blocks(F), stream, pos, faces, face_chart, chart_class, V, F, C, box_keys);
  return mesh_done();
}

extern "C" int gip_uv_place(const float* pos, const int32_t* vmapping, const int32_t* vt_chart, const int32_t* chart_class,
                            const float* chart_origin, int64_t V, int64_t Vt, int64_t C, float scale, int32_t texture_size, float* v_tex,
                            void* stream) {
  if (!mesh_count_ok(V) || !mesh_count_ok(Vt) || !mesh_count_ok(C) || texture_size < 1 || texture_size > 16384 ||
      !(scale > 0.f)) return 1;
  if (Vt == 0) return 0;
  if (!pos || !vmapping || !vt_chart || !chart_class || !chart_origin || !v_tex) return 1;
  MESH_LAUNCH(uv_place_kernel, mesh_blocks(Vt), stream, pos, vmapping, vt_chart, chart_class, chart_origin, V, Vt, C, scale,
            (float)texture_size, v_tex);
  return mesh_done();
}

extern "C" int gip_uv_vertex_tangents(const float* pos, const int32_t* faces, const int32_t* corner_start, const int32_t* corner_list,
                                      const int32_t* tex_idx, const float* v_tex, const float* nrm, int64_t V, int64_t F, int64_t Vt,
                                      float* face_tangents, float* tangents, void* stream) {
  if (!mesh_sizes_ok(V, F) || !mesh_count_ok(Vt)) return 1;
  if (V == 0) return 0;
  if (!pos || !corner_start || !nrm || !tangents || (F > 0 && (!faces || !corner_list || !tex_idx || !v_tex || !face_tangents))) return 1;
  if (F > 0) MESH_LAUNCH(uv_tangent_face_kernel, mesh_blocks(F), stream, pos, faces, tex_idx, v_tex, V, F, Vt, face_tangents);
  MESH_LAUNCH(uv_tangent_vertex_kernel, mesh_blocks(V), stream, corner_start, corner_list, (const float*)face_tangents, nrm, V, F, tangents);
  return mesh_done();
}

extern "C" int gip_uv_vertex_tangents_backward(const int32_t* faces, const int32_t* corner_start, const int32_t* corner_list,
                                               const int32_t* tex_idx, const float* v_tex, const float* nrm, const float* face_tangents,
                                               const float* g_tangents, int64_t V, int64_t F, int64_t Vt, float* g_sum, float* g_edge,
                                               float* g_pos, float* g_nrm, void* stream) {
  if (!mesh_sizes_ok(V, F) || !mesh_count_ok(Vt)) return 1;
  if (V == 0) return 0;
  if (!corner_start || !nrm || !g_tangents || !g_sum || !g_pos || !g_nrm ||
      (F > 0 && (!faces || !corner_list || !tex_idx || !v_tex || !face_tangents || !g_edge))) return 1;
  MESH_LAUNCH(uv_tangent_vertex_backward_kernel, mesh_blocks(V), stream, corner_start, corner_list, face_tangents, nrm, g_tangents, V, F, g_sum,
            g_nrm);
  if (F > 0) MESH_LAUNCH(uv_tangent_face_backward_kernel, mesh_blocks(F), stream, faces, tex_idx, v_tex, (const float*)g_sum, V, F, Vt, g_edge);
  MESH_LAUNCH(uv_tangent_gather_backward_kernel, mesh_blocks(V), stream, corner_start, corner_list, (const float*)g_edge, V, F, g_pos);
  return mesh_done();
}

extern "C" int gip_texture_dilate(float* tex_a, uint8_t* mask_a, float* tex_b, uint8_t* mask_b, int32_t H, int32_t W, int32_t C,
                                  int32_t rounds, void* stream) {
  if (H < 1 || W < 1 || H > 16384 || W > 16384 || C < 1 || C > 64 || (int64_t)H * W * C > INT32_MAX || rounds < 0 || rounds > 1024)
    return 1;
  if (rounds == 0) return 0;
  if (!tex_a || !mask_a || !tex_b || !mask_b) return 1;
  const int64_t blocks = mesh_blocks((int64_t)H * W);
  for (int r = 0; r < rounds; r++) {
    if (r & 1)
      MESH_LAUNCH(uv_dilate_kernel, blocks, stream, (const float*)tex_b, (const uint8_t*)mask_b, H, W, C, tex_a, mask_a);
    else
      MESH_LAUNCH(uv_dilate_kernel, blocks, stream, (const float*)tex_a, (const uint8_t*)mask_a, H, W, C, tex_b, mask_b);
  }
  return mesh_done();
}
