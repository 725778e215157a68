// mesh_geom.hip — the geometry terms of a mesh-fitting loop (threestudio/models/mesh.py: Mesh.v_nrm, Mesh.laplacian(),
// Mesh.normal_consistency()) with their backward passes, linked into libgip_model.so.  One mesh, pos [V, 3] float32 in object space.
//
// Everything is a GATHER over a connectivity table built once per face list (gaussianip_amd/utils/mesh_geometry.py MeshTopology):
//   corner_start [V + 1], corner_list [3 F]   the corners 3 f + k grouped by the vertex they name, ascending inside a group
//   nbr_start [V + 1], nbr_list [N]           per vertex its distinct neighbours j != i over all face edges, ascending
// One lane owns one vertex and walks its row in the table's order, so there is no float atomic anywhere and forward and backward are
// bitwise equal from run to run, whatever the valence (a row longer than a wave is the same loop).  The reference scatters instead
// (three scatter_add_, a sparse mm, autograd's index_add), whose float atomics on a GPU are not reproducible.
//
// Definitions.
//   vertex normals   s_v = sum over the corners of v, in corner_list order, of cross(p1 - p0, p2 - p0) of the corner's face;
//                    n_v = s_v / max(|s_v|, 1e-12) where dot(s_v, s_v) > 1e-20, else (0, 0, 1) (the reference's torch.where and then
//                    F.normalize).  len_v = |s_v|, and 0 where the default was taken: dot > 1e-20 means |s_v| >= 1e-10, so 0 marks it.
//                    A per-face pass writes the cross products to the caller's face_normals [F, 3] first and the gather reads them:
//                    12 bytes per corner instead of three indices and three positions (recomputing the cross product per corner
//                    gave the same bits and measured slower: DESIGN.md "Geometry terms of the mesh").
//       backward     g_s = (g_n - n (n . g_n)) / len, 0 where the default was taken; then per vertex over its corners, with
//                    g_face = g_s[i0] + g_s[i1] + g_s[i2] of the corner's face: corner 1 takes (p2 - p0) x g_face, corner 2
//                    g_face x (p1 - p0), corner 0 minus their sum.
//   Laplacian loss   Lp_v = deg_v p_v - sum_{j in nbr(v)} p_j, evaluated as sum_j (p_v - p_j): the differences of neighbouring
//                    positions are small and nearly exact, where deg p - sum p cancels two numbers of the mesh's size.
//                    loss = mean_v |Lp_v| over all V (an isolated vertex adds 0).  Kept for the backward: unit_v = Lp_v / |Lp_v|, 0
//                    where |Lp_v| == 0 (torch's norm has that subgradient).
//       backward     g_pos_v = (g / V) sum_j (unit_v - unit_j): L is symmetric, so it is the same gather.
//   consistency      loss = (1 / E) sum over the edges (a, b), a != b, of 1 - cos(n_a, n_b), each edge taking half from either end's
//                    row; cos = a . b / (max(|a|, 1e-8) max(|b|, 1e-8)).  E counts the pairs (a, a) of faces with a repeated index.
//       backward     g_n_v = -(g / E) sum_j d cos(n_v, n_j) / d n_v, d cos / d a = (b / |b| - cos a / |a|) / |a| with the lengths as
//                    computed (clamped), as the reference's autograd differentiates through them.
// The two means: per-workgroup partial sums (a fixed shuffle tree) into the caller's workspace, then one finishing workgroup adds
// them in index order in double.  Losses are device scalars; nothing is read back.
//
// Built with -ffp-contract=off.  Indices are trusted no further than memory safety needs: a corner, a face index or a neighbour
// outside its table is skipped, and a row is clamped to its list.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gip_model.h"
#include "mesh_common.h"

// the workgroup's sum of `value` to partial[blockIdx.x], in one fixed order
__device__ __forceinline__ void mg_block_sum(float value, float* __restrict__ partial) {
  __shared__ float s_red[MESH_THREADS / 64];
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) value += __shfl_xor(value, d, 64);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = value;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}

__global__ void __launch_bounds__(MESH_THREADS)
mesh_geom_face_normals_kernel(const float* __restrict__ pos, const int32_t* __restrict__ faces, int64_t V, int64_t F,
                              float* __restrict__ face_normals) {
  const int64_t f = (int64_t)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (f < F) mesh_store(face_normals, f, mesh_face_cross(pos, faces, f, V));
}

__global__ void __launch_bounds__(MESH_THREADS)
mesh_geom_normals_kernel(const int32_t* __restrict__ corner_start, const int32_t* __restrict__ corner_list,
                         const float* __restrict__ face_normals, int64_t V, int64_t F, float* __restrict__ n, float* __restrict__ len) {
  const int64_t v = (int64_t)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (v >= V) return;
  int64_t lo, hi;
  mesh_row(corner_start, v, 3 * F, &lo, &hi);
  MeshVec s = MeshVec{0.f, 0.f, 0.f};
  for (int64_t at = lo; at < hi; at++) {
    const int64_t c = corner_list[at];
    if ((uint64_t)c >= (uint64_t)(3 * F)) continue;
    s = mesh_add(s, mesh_load(face_normals, c / 3));
  }
  const float d = mesh_dot(s, s);
  if (d > 1e-20f) {
    const float l = sqrtf(d);
    const float q = fmaxf(l, 1e-12f);
    mesh_store(n, v, mesh_div(s, q));
    len[v] = l;
  } else {
    mesh_store(n, v, MeshVec{0.f, 0.f, 1.f});
    len[v] = 0.f;
  }
}

// g_s = (g_n - n (n . g_n)) / len through the normalisation; 0 where the default normal was taken
__global__ void __launch_bounds__(MESH_THREADS)
mesh_geom_normalize_backward_kernel(const float* __restrict__ n, const float* __restrict__ len, const float* __restrict__ g_n, int64_t V,
                                    float* __restrict__ g_s) {
  const int64_t v = (int64_t)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (v >= V) return;
  const float l = len[v];
  MeshVec out = MeshVec{0.f, 0.f, 0.f};
  if (l > 0.f) {
    const MeshVec nv = mesh_load(n, v), g = mesh_load(g_n, v);
    const MeshVec t = mesh_sub(g, mesh_scale(nv, mesh_dot(nv, g)));
    const float q = fmaxf(l, 1e-12f);
    out = mesh_div(t, q);
  }
  mesh_store(g_s, v, out);
}

__global__ void __launch_bounds__(MESH_THREADS)
mesh_geom_normals_backward_kernel(const float* __restrict__ pos, const int32_t* __restrict__ faces, const int32_t* __restrict__ corner_start,
                                  const int32_t* __restrict__ corner_list, const float* __restrict__ g_s, int64_t V, int64_t F,
                                  float* __restrict__ g_pos) {
  const int64_t v = (int64_t)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (v >= V) return;
  int64_t lo, hi;
  mesh_row(corner_start, v, 3 * F, &lo, &hi);
  MeshVec acc = MeshVec{0.f, 0.f, 0.f};
  for (int64_t at = lo; at < hi; at++) {
    const int64_t c = corner_list[at];
    if ((uint64_t)c >= (uint64_t)(3 * F)) continue;
    const int64_t f = c / 3;
    const int k = (int)(c - 3 * f);
    int32_t i0, i1, i2;
    if (!mesh_face(faces, f, V, &i0, &i1, &i2)) continue;
    const MeshVec g = mesh_add(mesh_add(mesh_load(g_s, i0), mesh_load(g_s, i1)), mesh_load(g_s, i2));
    const MeshVec p0 = mesh_load(pos, i0);
    const MeshVec e1 = mesh_sub(mesh_load(pos, i1), p0), e2 = mesh_sub(mesh_load(pos, i2), p0);
    acc = mesh_add(acc, mesh_corner_share(k, mesh_cross(e2, g), mesh_cross(g, e1)));
  }
  mesh_store(g_pos, v, acc);
}

__global__ void __launch_bounds__(MESH_THREADS)
mesh_geom_laplacian_kernel(const float* __restrict__ pos, const int32_t* __restrict__ nbr_start, const int32_t* __restrict__ nbr_list,
                           int64_t V, int64_t N, float* __restrict__ unit, float* __restrict__ partial) {
  const int64_t v = (int64_t)blockIdx.x * MESH_THREADS + threadIdx.x;
  float norm = 0.f;
  if (v < V) {
    int64_t lo, hi;
    mesh_row(nbr_start, v, N, &lo, &hi);
    const MeshVec p = mesh_load(pos, v);
    MeshVec lp = MeshVec{0.f, 0.f, 0.f};
    for (int64_t at = lo; at < hi; at++) {
      const int64_t j = nbr_list[at];
      if ((uint64_t)j >= (uint64_t)V) continue;
      lp = mesh_add(lp, mesh_sub(p, mesh_load(pos, j)));
    }
    norm = sqrtf(mesh_dot(lp, lp));
    mesh_store(unit, v, norm > 0.f ? mesh_div(lp, norm) : MeshVec{0.f, 0.f, 0.f});
  }
  mg_block_sum(norm, partial);
}

__global__ void __launch_bounds__(MESH_THREADS)
mesh_geom_laplacian_backward_kernel(const float* __restrict__ unit, const int32_t* __restrict__ nbr_start,
                                    const int32_t* __restrict__ nbr_list, const float* __restrict__ g_loss, int64_t V, int64_t N,
                                    float* __restrict__ g_pos) {
  const int64_t v = (int64_t)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (v >= V) return;
  int64_t lo, hi;
  mesh_row(nbr_start, v, N, &lo, &hi);
  const MeshVec u = mesh_load(unit, v);
  MeshVec acc = MeshVec{0.f, 0.f, 0.f};
  for (int64_t at = lo; at < hi; at++) {
    const int64_t j = nbr_list[at];
    if ((uint64_t)j >= (uint64_t)V) continue;
    acc = mesh_add(acc, mesh_sub(u, mesh_load(unit, j)));
  }
  mesh_store(g_pos, v, mesh_scale(acc, g_loss[0] / (float)V));
}

__global__ void __launch_bounds__(MESH_THREADS)
mesh_geom_consistency_kernel(const float* __restrict__ n, const int32_t* __restrict__ nbr_start, const int32_t* __restrict__ nbr_list,
                             int64_t V, int64_t N, float* __restrict__ partial) {
  const int64_t v = (int64_t)blockIdx.x * MESH_THREADS + threadIdx.x;
  float sum = 0.f;
  if (v < V) {
    int64_t lo, hi;
    mesh_row(nbr_start, v, N, &lo, &hi);
    const MeshVec a = mesh_load(n, v);
    const float la = fmaxf(sqrtf(mesh_dot(a, a)), 1e-8f);
    for (int64_t at = lo; at < hi; at++) {
      const int64_t j = nbr_list[at];
      if ((uint64_t)j >= (uint64_t)V) continue;
      const MeshVec b = mesh_load(n, j);
      const float lb = fmaxf(sqrtf(mesh_dot(b, b)), 1e-8f);
      sum += 1.f - mesh_dot(a, b) / (la * lb);
    }
    sum *= 0.5f;      // the other half comes from the neighbour's row
  }
  mg_block_sum(sum, partial);
}

__global__ void __launch_bounds__(MESH_THREADS)
mesh_geom_consistency_backward_kernel(const float* __restrict__ n, const int32_t* __restrict__ nbr_start,
                                      const int32_t* __restrict__ nbr_list, const float* __restrict__ g_loss, int64_t V, int64_t N,
                                      double edges, float* __restrict__ g_n) {
  const int64_t v = (int64_t)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (v >= V) return;
  int64_t lo, hi;
  mesh_row(nbr_start, v, N, &lo, &hi);
  const MeshVec a = mesh_load(n, v);
  const float la = fmaxf(sqrtf(mesh_dot(a, a)), 1e-8f);
  const MeshVec ua = mesh_div(a, la);
  MeshVec acc = MeshVec{0.f, 0.f, 0.f};
  for (int64_t at = lo; at < hi; at++) {
    const int64_t j = nbr_list[at];
    if ((uint64_t)j >= (uint64_t)V) continue;
    const MeshVec b = mesh_load(n, j);
    const float lb = fmaxf(sqrtf(mesh_dot(b, b)), 1e-8f);
    const float c = mesh_dot(a, b) / (la * lb);
    acc = mesh_add(acc, mesh_sub(mesh_div(b, lb), mesh_scale(ua, c)));
  }
  const float s = -(g_loss[0] / (float)edges) / la;
  mesh_store(g_n, v, mesh_scale(acc, s));
}

// the mean: the partials in index order, in double, divided by count; one workgroup
__global__ void __launch_bounds__(MESH_THREADS)
mesh_geom_finish_kernel(const float* __restrict__ partial, int64_t blocks, double count, float* __restrict__ loss) {
  __shared__ double s_red[MESH_THREADS / 64];
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < blocks; i += MESH_THREADS) acc += (double)partial[i];
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 64);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) loss[0] = (float)(((s_red[0] + s_red[1]) + (s_red[2] + s_red[3])) / count);
}

extern "C" int gip_mesh_geometry_workspace_size(int64_t V, size_t* bytes) {
  if (!bytes || !mesh_count_ok(V)) return 1;
  *bytes = (size_t)mesh_blocks(V) * sizeof(float);
  return 0;
}

extern "C" int gip_mesh_vertex_normals(const float* pos, const int32_t* faces, const int32_t* corner_start, const int32_t* corner_list,
                                       int64_t V, int64_t F, float* face_normals, float* n, float* len, void* stream) {
  if (!mesh_sizes_ok(V, F)) return 1;
  if (V == 0 || F == 0) return 0;
  if (!pos || !faces || !corner_start || !corner_list || !face_normals || !n || !len) return 1;
  MESH_LAUNCH(mesh_geom_face_normals_kernel, mesh_blocks(F), stream, pos, faces, V, F, face_normals);
  MESH_LAUNCH(mesh_geom_normals_kernel, mesh_blocks(V), stream, corner_start, corner_list, (const float*)face_normals, V, F, n, len);
  return mesh_done();
}

extern "C" int gip_mesh_vertex_normals_backward(const float* pos, const int32_t* faces, const int32_t* corner_start,
                                                const int32_t* corner_list, const float* n, const float* len, const float* g_n, int64_t V,
                                                int64_t F, float* g_s, float* g_pos, void* stream) {
  if (!mesh_sizes_ok(V, F)) return 1;
  if (V == 0 || F == 0) return 0;
  if (!pos || !faces || !corner_start || !corner_list || !n || !len || !g_n || !g_s || !g_pos) return 1;
  MESH_LAUNCH(mesh_geom_normalize_backward_kernel, mesh_blocks(V), stream, n, len, g_n, V, g_s);
  MESH_LAUNCH(mesh_geom_normals_backward_kernel, mesh_blocks(V), stream, pos, faces, corner_start, corner_list, (const float*)g_s, V, F, g_pos);
  return mesh_done();
}

extern "C" int gip_mesh_laplacian_loss(const float* pos, const int32_t* nbr_start, const int32_t* nbr_list, int64_t V, int64_t N,
                                       float* unit, float* loss, void* workspace, size_t workspace_bytes, void* stream) {
  if (!mesh_count_ok(V) || !mesh_count_ok(N)) return 1;
  if (V == 0) return 0;
  if (!pos || !nbr_start || (N > 0 && !nbr_list) || !unit || !loss || !workspace) return 1;
  const int64_t blocks = mesh_blocks(V);
  if (workspace_bytes < (size_t)blocks * sizeof(float)) return 1;
  MESH_LAUNCH(mesh_geom_laplacian_kernel, blocks, stream, pos, nbr_start, nbr_list, V, N, unit, (float*)workspace);
  MESH_LAUNCH(mesh_geom_finish_kernel, 1, stream, (const float*)workspace, blocks, (double)V, loss);
  return mesh_done();
}

extern "C" int gip_mesh_laplacian_loss_backward(const float* unit, const int32_t* nbr_start, const int32_t* nbr_list, const float* g_loss,
                                                int64_t V, int64_t N, float* g_pos, void* stream) {
  if (!mesh_count_ok(V) || !mesh_count_ok(N)) return 1;
  if (V == 0) return 0;
  if (!unit || !nbr_start || (N > 0 && !nbr_list) || !g_loss || !g_pos) return 1;
  MESH_LAUNCH(mesh_geom_laplacian_backward_kernel, mesh_blocks(V), stream, unit, nbr_start, nbr_list, g_loss, V, N, g_pos);
  return mesh_done();
}

extern "C" int gip_mesh_normal_consistency(const float* n, const int32_t* nbr_start, const int32_t* nbr_list, int64_t V, int64_t N,
                                           int64_t E, float* loss, void* workspace, size_t workspace_bytes, void* stream) {
  if (!mesh_count_ok(V) || !mesh_count_ok(N) || E < 0) return 1;
  if (V == 0 || E == 0) return 0;
  if (!n || !nbr_start || (N > 0 && !nbr_list) || !loss || !workspace) return 1;
  const int64_t blocks = mesh_blocks(V);
  if (workspace_bytes < (size_t)blocks * sizeof(float)) return 1;
  MESH_LAUNCH(mesh_geom_consistency_kernel, blocks, stream, n, nbr_start, nbr_list, V, N, (float*)workspace);
  MESH_LAUNCH(mesh_geom_finish_kernel, 1, stream, (const float*)workspace, blocks, (double)E, loss);
  return mesh_done();
}

extern "C" int gip_mesh_normal_consistency_backward(const float* n, const int32_t* nbr_start, const int32_t* nbr_list, const float* g_loss,
                                                    int64_t V, int64_t N, int64_t E, float* g_n, void* stream) {
  if (!mesh_count_ok(V) || !mesh_count_ok(N) || E < 0) return 1;
  if (V == 0 || E == 0) return 0;
  if (!n || !nbr_start || (N > 0 && !nbr_list) || !g_loss || !g_n) return 1;
  MESH_LAUNCH(mesh_geom_consistency_backward_kernel, mesh_blocks(V), stream, n, nbr_start, nbr_list, g_loss, V, N, (double)E, g_n);
  return mesh_done();
}
