// mesh_clean.hip — cleaning and decimating the extracted triangle mesh on the GPU: connected components, per-component statistics,
// and vertex clustering on a grid with one quadric-optimal vertex per occupied cell (gaussianip_amd/utils/mesh.py; DESIGN.md
// "Cleaning and decimating the mesh").  Replaces the reference's calls of kiui's clean_mesh / decimate_mesh (gs_renderer.py:346-350).
// Linked into libgip_model.so.  No kernel here spins, waits on another workgroup or uses a grid-wide barrier; every loop over rounds
// lives on the host.
//
// Connected components.  label[v] starts as v (the caller's arange).  One round = mc_hook_kernel, then mc_compress_kernel, the scheme
//   of mesh_common.h "Labels", which proves that the fixed point is the component's smallest vertex whatever the interleaving:
//   hook      one lane per face: m = min(label[a], label[b], label[c]); for each corner x an integer atomicMin of m into
//             label[label[x]] and into label[x].  A face with an index outside [0, V) is skipped.
//   compress  one lane per vertex: mesh_label_compress.
//
// Statistics.  mc_stats_kernel, one lane per face: an integer atomicAdd into count[label] and atomicMin / atomicMax of its three
//   corners' coordinates into box[label], on mesh_common.h's float key.  Integer atomics only: order-independent.
//   mc_box_decode_kernel turns the keys back into floats (rows of components without a face are not defined).
//
// Clustering.  The grid: per axis i = min((int) floorf((p - lo) / h), n - 1), float32, that operand order, a correctly rounded
//   division; key = (iz n + iy) n + ix.  lo, h and n are the caller's (h = L / n in float32 on the host), so every kernel here and
//   the numpy restatement agree on membership exactly.  A coordinate below lo (not a vertex of the mesh the grid was made for) goes
//   to cell 0; a NaN likewise.
//   mc_keys_kernel    key of every vertex (int64).
//   mc_count_kernel   the faces whose three corners lie in three different cells, for the bisection of decimate_mesh; a wave adds
//                     its ballot's population with one integer atomicAdd.
//   mc_place_kernel   the hot path: a gather, no float atomics.  LPC lanes (16, 32 or 64) per occupied cell.  The caller passes the 3 F
//                     face corners stably sorted by the cell of the corner's vertex (corner_order, corner_start) and the vertices stably
//                     sorted by cell (member_order, member_start).  Lane j takes entries j, j + LPC, ... of the cell's run in that
//                     order, then the LPC partial sums are added in a butterfly (xor 1, 2, 4, ...): a fixed order and a fixed tree,
//                     so two runs are bit-identical.  All arithmetic in the cell's local coordinates q = (p - c) / h,
//                     c = lo + (i + 0.5) h: for a face (a, b, c), n = (q_b - q_a) x (q_c - q_a), w = |n|, skipped when w == 0,
//                         A += n n^T / w      b += n (n . q_a) / w      (each product divided by w, nothing precomputed)
//                     and the members' q summed into the mean m.  The vertex solves (A + l tr(A) I) x = b + l tr(A) m, l = 1e-3, by
//                     an LDL^T factorisation (the matrix is symmetric positive definite with a condition number <= 1 / l + 1), is
//                     clamped per axis to [-0.5, 0.5] and written as c + h x.  A cell with tr(A) == 0 gets m.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gip_model.h"
#include "mesh_common.h"

#define MC_MAX_GRID 2048
#define MC_LAMBDA 1e-3f

// ------------------------------------------------------------------------------------------------------------------ components
__global__ void __launch_bounds__(MESH_THREADS)
mc_hook_kernel(const int32_t* __restrict__ faces, int F, int V, int32_t* label, int32_t* __restrict__ changed) {
  const int f = blockIdx.x * MESH_THREADS + threadIdx.x;
  if (f >= F) return;
  int32_t a, b, c;
  if (!mesh_face(faces, f, V, &a, &b, &c)) return;
  // volatile reads: other lanes lower these words while this kernel runs; any value seen is a valid (later or earlier) label in [0, V)
  const int la = __atomic_load_n(label + a, __ATOMIC_RELAXED), lb = __atomic_load_n(label + b, __ATOMIC_RELAXED),
            lc = __atomic_load_n(label + c, __ATOMIC_RELAXED);
  const int m = min(la, min(lb, lc));
  bool moved = false;
  const int x[3] = {a, b, c}, lx[3] = {la, lb, lc};
#pragma unroll
  for (int k = 0; k < 3; k++) {
    if (lx[k] <= m) continue;
    if (atomicMin(label + lx[k], m) > m) moved = true;   // lx[k] in [0, V): it was read from label
    if (atomicMin(label + x[k], m) > m) moved = true;
  }
  if (moved) *changed = 1;
}

__global__ void __launch_bounds__(MESH_THREADS)
mc_compress_kernel(int V, int32_t* label, int32_t* __restrict__ changed) {
  mesh_label_compress(label, blockIdx.x * MESH_THREADS + threadIdx.x, V, changed);
}

// ------------------------------------------------------------------------------------------------------------------ statistics
__global__ void __launch_bounds__(MESH_THREADS)
mc_stats_init_kernel(int V, int32_t* __restrict__ count, uint32_t* __restrict__ box) {
  const int v = blockIdx.x * MESH_THREADS + threadIdx.x;
  if (v >= V) return;
  count[v] = 0;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    box[(int64_t)v * 6 + k] = 0xffffffffu;
    box[(int64_t)v * 6 + 3 + k] = 0u;
  }
}

__global__ void __launch_bounds__(MESH_THREADS)
mc_stats_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ faces, int F, int V, const int32_t* __restrict__ label,
                int32_t* __restrict__ count, uint32_t* __restrict__ box) {
  const int f = blockIdx.x * MESH_THREADS + threadIdx.x;
  if (f >= F) return;
  int32_t x[3];
  if (!mesh_face(faces, f, V, &x[0], &x[1], &x[2])) return;
  const int l = label[x[0]];
  if (l < 0 || l >= V) return;   // not a label of connected_components: nothing is written outside the arrays
  atomicAdd(count + l, 1);
#pragma unroll
  for (int k = 0; k < 3; k++)
#pragma unroll
    for (int ax = 0; ax < 3; ax++) {
      const uint32_t key = mesh_float_key(vertices[(int64_t)x[k] * 3 + ax]);
      atomicMin(box + (int64_t)l * 6 + ax, key);
      atomicMax(box + (int64_t)l * 6 + 3 + ax, key);
    }
}

__global__ void __launch_bounds__(MESH_THREADS)
mc_box_decode_kernel(int64_t N, uint32_t* __restrict__ box) {
  const int64_t i = (int64_t)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (i >= N) return;
  box[i] = __float_as_uint(mesh_key_float(box[i]));
}

// ------------------------------------------------------------------------------------------------------------------ the grid
__device__ __forceinline__ int mc_cell(float p, float lo, float h, int n) {
  const float t = floorf((p - lo) / h);
  if (!(t > 0.f)) return 0;               // below lo, or NaN
  return t >= (float)n ? n - 1 : (int)t;
}

__global__ void __launch_bounds__(MESH_THREADS)
mc_keys_kernel(const float* __restrict__ vertices, int V, float lox, float loy, float loz, float h, int n, int64_t* __restrict__ key) {
  const int v = blockIdx.x * MESH_THREADS + threadIdx.x;
  if (v >= V) return;
  const int ix = mc_cell(vertices[(int64_t)v * 3], lox, h, n), iy = mc_cell(vertices[(int64_t)v * 3 + 1], loy, h, n),
            iz = mc_cell(vertices[(int64_t)v * 3 + 2], loz, h, n);
  key[v] = ((int64_t)iz * n + iy) * n + ix;
}

__global__ void __launch_bounds__(MESH_THREADS)
mc_count_kernel(const float* __restrict__ vertices, int V, const int32_t* __restrict__ faces, int F, float lox, float loy, float loz, float h,
                int n, int32_t* __restrict__ count) {
  const int f = blockIdx.x * MESH_THREADS + threadIdx.x;
  bool alive = false;
  if (f < F) {
    int32_t x[3];
    if (mesh_face(faces, f, V, &x[0], &x[1], &x[2])) {
      int64_t k[3];
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const float* p = vertices + (int64_t)x[c] * 3;
        k[c] = ((int64_t)mc_cell(p[2], loz, h, n) * n + mc_cell(p[1], loy, h, n)) * n + mc_cell(p[0], lox, h, n);
      }
      alive = k[0] != k[1] && k[1] != k[2] && k[0] != k[2];
    }
  }
  const uint64_t bal = __ballot(alive);
  if ((threadIdx.x & 63) == 0 && bal) atomicAdd(count, __popcll(bal));
}

// ------------------------------------------------------------------------------------------------------------------ placement
template <int LPC>
__global__ void __launch_bounds__(MESH_THREADS)
mc_place_kernel(const float* __restrict__ vertices, int V, const int32_t* __restrict__ faces, int F, const int64_t* __restrict__ cell_key, int C,
                const int32_t* __restrict__ corner_order, const int32_t* __restrict__ corner_start, const int32_t* __restrict__ member_order,
                const int32_t* __restrict__ member_start, float lox, float loy, float loz, float h, int n, float* __restrict__ out) {
  const int cell = (int)(((int64_t)blockIdx.x * MESH_THREADS + threadIdx.x) / LPC), j = threadIdx.x & (LPC - 1);
  // a cell past the end does the arithmetic on empty runs (the shuffles below need whole groups) and writes nothing
  const bool live = cell < C;
  const int64_t key = live ? cell_key[cell] : 0;
  const int ix = (int)(key % n), iy = (int)((key / n) % n), iz = (int)(key / ((int64_t)n * n));
  const float cx = lox + ((float)ix + 0.5f) * h, cy = loy + ((float)iy + 0.5f) * h, cz = loz + ((float)iz + 0.5f) * h;
  // the run's ends clipped to the arrays: whatever the caller wrote there, nothing outside them is read
  const int e0 = live ? min(max(corner_start[cell], 0), 3 * F) : 0, e1 = live ? min(max(corner_start[cell + 1], 0), 3 * F) : 0;
  const int m0 = live ? min(max(member_start[cell], 0), V) : 0, m1 = live ? min(max(member_start[cell + 1], 0), V) : 0;
  float acc[13];   // A: xx xy xz yy yz zz; b: x y z; members: x y z count
#pragma unroll
  for (int k = 0; k < 13; k++) acc[k] = 0.f;
  for (int e = e0 + j; e < e1; e += LPC) {
    const int f = corner_order[e] / 3;
    if (f < 0 || f >= F) continue;
    const int a = faces[(int64_t)f * 3], b = faces[(int64_t)f * 3 + 1], c = faces[(int64_t)f * 3 + 2];
    if (a < 0 || a >= V || b < 0 || b >= V || c < 0 || c >= V) continue;
    const float* pa = vertices + (int64_t)a * 3;
    const float* pb = vertices + (int64_t)b * 3;
    const float* pc = vertices + (int64_t)c * 3;
    const float ax = (pa[0] - cx) / h, ay = (pa[1] - cy) / h, az = (pa[2] - cz) / h;
    const float bx = (pb[0] - cx) / h, by = (pb[1] - cy) / h, bz = (pb[2] - cz) / h;
    const float qx = (pc[0] - cx) / h, qy = (pc[1] - cy) / h, qz = (pc[2] - cz) / h;
    const float ux = bx - ax, uy = by - ay, uz = bz - az, vx = qx - ax, vy = qy - ay, vz = qz - az;
    const float nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
    const float w = sqrtf(nx * nx + ny * ny + nz * nz);
    if (!(w > 0.f)) continue;
    const float d = nx * ax + ny * ay + nz * az;
    acc[0] += (nx * nx) / w;
    acc[1] += (nx * ny) / w;
    acc[2] += (nx * nz) / w;
    acc[3] += (ny * ny) / w;
    acc[4] += (ny * nz) / w;
    acc[5] += (nz * nz) / w;
    acc[6] += (nx * d) / w;
    acc[7] += (ny * d) / w;
    acc[8] += (nz * d) / w;
  }
  for (int e = m0 + j; e < m1; e += LPC) {
    const int v = member_order[e];
    if (v < 0 || v >= V) continue;
    acc[9] += (vertices[(int64_t)v * 3] - cx) / h;
    acc[10] += (vertices[(int64_t)v * 3 + 1] - cy) / h;
    acc[11] += (vertices[(int64_t)v * 3 + 2] - cz) / h;
    acc[12] += 1.f;
  }
#pragma unroll
  for (int off = 1; off < LPC; off <<= 1)
#pragma unroll
    for (int k = 0; k < 13; k++) acc[k] += __shfl_xor(acc[k], off, LPC);
  if (!live || j != 0) return;
  const float cnt = acc[12] > 0.f ? acc[12] : 1.f;
  const float mx = acc[9] / cnt, my = acc[10] / cnt, mz = acc[11] / cnt;
  float x = mx, y = my, z = mz;
  const float tr = acc[0] + acc[3] + acc[5];
  if (tr > 0.f) {
    const float r = MC_LAMBDA * tr;
    const float a00 = acc[0] + r, a01 = acc[1], a02 = acc[2], a11 = acc[3] + r, a12 = acc[4], a22 = acc[5] + r;
    const float r0 = acc[6] + r * mx, r1 = acc[7] + r * my, r2 = acc[8] + r * mz;
    // LDL^T: every pivot is >= l tr(A) > 0
    const float l10 = a01 / a00, l20 = a02 / a00;
    const float d1 = a11 - l10 * a01;
    const float t12 = a12 - l20 * a01;
    const float l21 = t12 / d1;
    const float d2 = a22 - l20 * a02 - l21 * t12;
    const float y0 = r0, y1 = r1 - l10 * y0, y2 = r2 - l20 * y0 - l21 * y1;
    z = y2 / d2;
    y = y1 / d1 - l21 * z;
    x = y0 / a00 - l10 * y - l20 * z;
  }
  x = fminf(fmaxf(x, -0.5f), 0.5f);
  y = fminf(fmaxf(y, -0.5f), 0.5f);
  z = fminf(fmaxf(z, -0.5f), 0.5f);
  out[(int64_t)cell * 3] = cx + h * x;
  out[(int64_t)cell * 3 + 1] = cy + h * y;
  out[(int64_t)cell * 3 + 2] = cz + h * z;
}

// ------------------------------------------------------------------------------------------------------------------ entry points
static int mc_grid_ok(float h, int32_t n) { return n >= 1 && n <= MC_MAX_GRID && h > 0.f && h <= 3.0e38f; }

// workgroups for a count that may pass INT32_MAX (6 V box words, C * lanes placement lanes), which mesh_blocks refuses
static int64_t mc_wide_blocks(int64_t items) { return (items + MESH_THREADS - 1) / MESH_THREADS; }

extern "C" int gip_mesh_components_rounds(const int32_t* faces, int64_t F, int64_t V, int32_t* labels, int32_t* changed, int32_t rounds,
                                          void* stream) {
  if (!mesh_sizes_ok(V, F) || rounds < 1 || rounds > 64) return 1;
  if (F == 0 || V == 0) return 0;
  if (!faces || !labels || !changed) return 1;
  for (int r = 0; r < rounds; r++) {
    MESH_LAUNCH(mc_hook_kernel, mesh_blocks(F), stream, faces, (int)F, (int)V, labels, changed);
    MESH_LAUNCH(mc_compress_kernel, mesh_blocks(V), stream, (int)V, labels, changed);
  }
  return mesh_done();
}

extern "C" int gip_mesh_component_stats(const float* vertices, const int32_t* faces, int64_t F, int64_t V, const int32_t* labels,
                                        int32_t* face_count, float* box, void* stream) {
  if (!mesh_sizes_ok(V, F)) return 1;
  if (V == 0) return 0;
  if (!face_count || !box) return 1;
  if (F > 0 && (!vertices || !faces || !labels)) return 1;
  MESH_LAUNCH(mc_stats_init_kernel, mesh_blocks(V), stream, (int)V, face_count, (uint32_t*)box);
  if (F > 0) MESH_LAUNCH(mc_stats_kernel, mesh_blocks(F), stream, vertices, faces, (int)F, (int)V, labels, face_count, (uint32_t*)box);
  MESH_LAUNCH(mc_box_decode_kernel, mc_wide_blocks(V * 6), stream, V * 6, (uint32_t*)box);
  return mesh_done();
}

extern "C" int gip_mesh_cluster_keys(const float* vertices, int64_t V, float lo_x, float lo_y, float lo_z, float h, int32_t n, int64_t* keys,
                                     void* stream) {
  if (!mesh_count_ok(V) || !mc_grid_ok(h, n)) return 1;
  if (V == 0) return 0;
  if (!vertices || !keys) return 1;
  MESH_LAUNCH(mc_keys_kernel, mesh_blocks(V), stream, vertices, (int)V, lo_x, lo_y, lo_z, h, (int)n, keys);
  return mesh_done();
}

extern "C" int gip_mesh_cluster_count(const float* vertices, int64_t V, const int32_t* faces, int64_t F, float lo_x, float lo_y, float lo_z,
                                      float h, int32_t n, int32_t* count, void* stream) {
  if (!mesh_sizes_ok(V, F) || !mc_grid_ok(h, n) || !count) return 1;
  if (F > 0 && (!vertices || !faces || V == 0)) return 1;
  if (hipMemsetAsync(count, 0, sizeof(int32_t), (hipStream_t)stream) != hipSuccess) return 3;
  if (F == 0) return 0;
  MESH_LAUNCH(mc_count_kernel, mesh_blocks(F), stream, vertices, (int)V, faces, (int)F, lo_x, lo_y, lo_z, h, (int)n, count);
  return mesh_done();
}

extern "C" int gip_mesh_cluster_place(const float* vertices, int64_t V, const int32_t* faces, int64_t F, const int64_t* cell_key, int64_t C,
                                      const int32_t* corner_order, const int32_t* corner_start, const int32_t* member_order,
                                      const int32_t* member_start, float lo_x, float lo_y, float lo_z, float h, int32_t n, int32_t lanes,
                                      float* out, void* stream) {
  if (!mesh_sizes_ok(V, F) || !mc_grid_ok(h, n) || C < 0 || C > V) return 1;
  if (lanes != 16 && lanes != 32 && lanes != 64) return 1;
  if (C == 0) return 0;
  if (!vertices || !cell_key || !corner_start || !member_order || !member_start || !out) return 1;
  if (F > 0 && (!faces || !corner_order)) return 1;
#define MC_PLACE(L)                                                                                                                    \
  MESH_LAUNCH((mc_place_kernel<L>), mc_wide_blocks(C * lanes), stream, vertices, (int)V, faces, (int)F, cell_key, (int)C, corner_order, \
              corner_start, member_order, member_start, lo_x, lo_y, lo_z, h, (int)n, out)
  if (lanes == 16) MC_PLACE(16);
  else if (lanes == 32) MC_PLACE(32);
  else MC_PLACE(64);
#undef MC_PLACE
  return mesh_done();
}
