// mesh_common.h — the vocabulary the mesh kernel files share (mesh_geom.hip, mesh_uv.hip, mesh_clean.hip and, through
// mesh_raster_common.h, the rasterizer trio): a three-float vector, a face's checked indices, a table row, the float key, the label
// compress and the host tail of an entry point.  Device functions are inlined and host functions static: the files link into one
// library, so nothing here is a __global__.  All of them are compiled with -ffp-contract=off: every operation below is the one
// correctly rounded float32 operation written, a division stays a division, and a sum runs left to right.
//
// The float key.  mesh_float_key is the order-preserving 32-bit image of a float: bits | 0x80000000 for a non-negative value, ~bits
//   for a negative one, -0 counting as +0; mesh_key_float is its inverse.  a < b exactly when key(a) < key(b), so a minimum or maximum
//   of floats is an integer atomicMin / atomicMax of keys: exact, and therefore independent of the order of the atomics.
//
// Labels.  Min-label propagation with pointer jumping over a graph of n items (mesh_clean.hip: vertices joined by faces; mesh_uv.hip:
//   faces of one class joined across edges).  label[i] starts as i.  One round = the file's hook kernel, which for every edge lowers the
//   labels at its ends, and the words those labels name, to the smallest label it read there by integer atomicMin; then a compress
//   kernel around mesh_label_compress, one lane per item: label[i] = the end of the chain i -> label[i] -> label[label[i]] -> ...
//   Either raises *changed when it lowered a label, and the host stops after rounds that changed nothing.
//   Why the fixed point is the component's minimum.  Three invariants hold at every moment, whatever the interleaving: (1) labels only
//   decrease (every write is an atomicMin of a value read from label); (2) label[i] <= i (true at the start, kept by 1), so every chain
//   is strictly decreasing until it reaches an r with label[r] == r, and the compress loop ends after at most n steps; (3) label[i]
//   names an item of i's own component (a hook copies a label between the ends of one edge or onto the item that one of them names,
//   compress follows names).  When a round changes nothing, the ends of every edge carry one label (else the hook's atomicMin would
//   have lowered one) and every label is a root (else compress would have moved it); labels are therefore constant on a component, the
//   common value r is a member of it by 3 and r <= every member by 2: r is the minimum.  Races change the number of rounds, never the
//   result.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define MESH_THREADS 256

struct MeshVec { float x, y, z; };

__device__ __forceinline__ MeshVec mesh_load(const float* __restrict__ p, int64_t i) { return MeshVec{p[3 * i], p[3 * i + 1], p[3 * i + 2]}; }
__device__ __forceinline__ void mesh_store(float* __restrict__ p, int64_t i, MeshVec v) { p[3 * i] = v.x; p[3 * i + 1] = v.y; p[3 * i + 2] = v.z; }
__device__ __forceinline__ MeshVec mesh_add(MeshVec a, MeshVec b) { return MeshVec{a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ MeshVec mesh_sub(MeshVec a, MeshVec b) { return MeshVec{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ MeshVec mesh_scale(MeshVec a, float s) { return MeshVec{a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ MeshVec mesh_div(MeshVec a, float s) { return MeshVec{a.x / s, a.y / s, a.z / s}; }
__device__ __forceinline__ MeshVec mesh_neg(MeshVec a) { return MeshVec{-a.x, -a.y, -a.z}; }
__device__ __forceinline__ float mesh_dot(MeshVec a, MeshVec b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ MeshVec mesh_cross(MeshVec a, MeshVec b) {
  return MeshVec{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ float mesh_comp(MeshVec v, int axis) { return axis == 0 ? v.x : (axis == 1 ? v.y : v.z); }

// a face's three indices; false when one lies outside [0, V)
__device__ __forceinline__ bool mesh_face(const int32_t* __restrict__ faces, int64_t f, int64_t V, int32_t* i0, int32_t* i1, int32_t* i2) {
  *i0 = faces[3 * f];
  *i1 = faces[3 * f + 1];
  *i2 = faces[3 * f + 2];
  return (uint64_t)*i0 < (uint64_t)V && (uint64_t)*i1 < (uint64_t)V && (uint64_t)*i2 < (uint64_t)V;
}

// cross(p1 - p0, p2 - p0) of face f, not normalised; 0 for a face with an index outside [0, V)
__device__ __forceinline__ MeshVec mesh_face_cross(const float* __restrict__ pos, const int32_t* __restrict__ faces, int64_t f, int64_t V) {
  int32_t i0, i1, i2;
  if (!mesh_face(faces, f, V, &i0, &i1, &i2)) return MeshVec{0.f, 0.f, 0.f};
  const MeshVec p0 = mesh_load(pos, i0);
  return mesh_cross(mesh_sub(mesh_load(pos, i1), p0), mesh_sub(mesh_load(pos, i2), p0));
}

// the row [start[v], start[v + 1]) of a table of `total` entries, clamped to it
__device__ __forceinline__ void mesh_row(const int32_t* __restrict__ start, int64_t v, int64_t total, int64_t* lo, int64_t* hi) {
  int64_t a = start[v], b = start[v + 1];
  a = a < 0 ? 0 : a;
  b = b > total ? total : b;
  *lo = a;
  *hi = b;
}

// what corner k of a face takes of the gradients g1, g2 to its edges p1 - p0 and p2 - p0: corner 1 g1, corner 2 g2, corner 0 minus their sum
__device__ __forceinline__ MeshVec mesh_corner_share(int k, MeshVec g1, MeshVec g2) {
  if (k == 1) return g1;
  if (k == 2) return g2;
  return mesh_neg(mesh_add(g1, g2));
}

__device__ __forceinline__ uint32_t mesh_float_key(float d) {
  uint32_t u = __float_as_uint(d);
  if ((u & 0x7fffffffu) == 0) u = 0;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float mesh_key_float(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? (u ^ 0x80000000u) : ~u); }

// one lane's compress of item i of n ("Labels" above); a word outside [0, n) ends the chain, so nothing outside label is read
__device__ __forceinline__ void mesh_label_compress(int32_t* label, int i, int n, int32_t* __restrict__ changed) {
  if (i >= n) return;
  const int first = __atomic_load_n(label + i, __ATOMIC_RELAXED);
  int l = first;
  // strictly decreasing (label[x] <= x always): at most n steps, whatever other lanes store meanwhile
  for (int step = 0; step < n; step++) {
    if (l < 0 || l >= n) break;
    const int next = __atomic_load_n(label + l, __ATOMIC_RELAXED);
    if (next >= l || next < 0) break;
    l = next;
  }
  if (l < first && l >= 0) {
    atomicMin(label + i, l);
    *changed = 1;
  }
}

// ------------------------------------------------------------------------------------------------------------------------ host
static bool mesh_count_ok(int64_t n) { return n >= 0 && n <= INT32_MAX; }

// V vertices and F faces whose 3 F corners are indexed in int32
static bool mesh_sizes_ok(int64_t V, int64_t F) { return mesh_count_ok(V) && F >= 0 && F <= INT32_MAX / 3; }

// workgroups of one lane per item; 0 when the count is not launchable
static int64_t mesh_blocks(int64_t items) {
  if (items < 1 || items > INT32_MAX) return 0;
  return (items + MESH_THREADS - 1) / MESH_THREADS;
}

#define MESH_LAUNCH(kernel, blocks, stream, ...) \
  hipLaunchKernelGGL(kernel, dim3((unsigned)(blocks)), dim3(MESH_THREADS), 0, (hipStream_t)(stream), __VA_ARGS__)

// an entry point's status after its launches
static int mesh_done(void) { return hipGetLastError() == hipSuccess ? 0 : 3; }
