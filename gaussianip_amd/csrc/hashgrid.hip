// hashgrid.hip — a multiresolution hash-grid encoding of 3-D points (the published Instant-NGP scheme: Mueller et al. 2022, "Instant
// Neural Graphics Primitives with a Multiresolution Hash Encoding"), forward and both backward passes.  It is what the reference gets
// from tinycudann (threestudio/models/networks.py:55-106, TCNNEncoding with otype HashGrid); tinycudann is CUDA-only, so the definition
// below is the project's own reading of the scheme.  Its table layout has not been checked against a tinycudann checkpoint.
// Linked into libgip_model.so; gaussianip_amd/utils/encoding.py is the host side.
//
// Definition.  x [N, 3] float32, meant to lie in [0, 1]; table [P, F] float32, one slice of rows per level; L levels (1 .. 32), F
// features per level (1, 2, 4 or 8).  The level table is computed ONCE on the host (encoding.py HashGridLayout) and handed to every entry
// point as arrays, so the kernels and the tests' restatement cannot disagree on it:
//   scale_l  = exp2f(l * log2f(per_level_scale)) * base_resolution - 1            float32
//   res_l    = ceil(scale_l) + 1
//   size_l   = min(round_up(res_l^3, 8), 2^log2_hashmap_size)   (a cube above 2^log2_hashmap_size counts as too large), at most 2^24
//   offset_l = the running sum of the sizes; P = their total
//   hashed_l = res_l^3 > size_l
// Per point and level, in float32 with every operation rounded on its own (-ffp-contract=off):
//   pos = x * scale_l + 0.5, cell = floor(pos), frac = pos - cell                 per axis
//   the eight corners cell + {0, 1}^3 (corner k: bit 0 = +x, bit 1 = +y, bit 2 = +z) weigh prod_axes (bit ? frac : 1 - frac)
//   a corner's row, in uint32 arithmetic on the corner's coordinates (a negative one wraps):
//       dense   cx + cy * res_l + cz * res_l^2
//       hashed  cx ^ (cy * 2654435761) ^ (cz * 805459861)
//     and in both cases reduced % size_l, which is also what keeps x = 1 and inputs outside [0, 1] inside the slice.
//   A point with |pos| >= 2^30 on some axis of a level, or a pos that is not finite (a NaN or an infinite coordinate), gets a zero output
//   row on that level and contributes no gradient there; no index is formed from it.
//   enc[n, l F + f] = sum over the corners in the order k = 0 .. 7 of w_k * table[offset_l + row_k, f]                [N, L F], level-major
// Gradients (first order only):
//   g_table[offset_l + row_k, f] += w_k * g[n, l F + f]
//   g_x[n, axis] = sum over levels in level order of scale_l * sum over the four corner pairs across that axis of (the weights of the
//                  other two axes) * (d_hi - d_lo), with d_k = sum_f g[n, l F + f] * table[offset_l + row_k, f]
//
// Kernels (wave64).  hashgrid_forward_kernel and hashgrid_backward_table_kernel take one lane per (point, level) with the level as the
// slow grid axis: at any moment the chip works on few levels, and a slice of at most 2^19 rows x 8 B stays in L2 while its points go
// through.  A corner's F features are one load of 4 F bytes.  hashgrid_backward_input_kernel is a gather with the same walk, one lane per
// point summing its levels in level order.  Forward and the gradient to x use no atomics and are bitwise equal from run to run.
// NOT reproducible: g_table.  The scatter adds with atomicAdd(float*), which compiles to one no-return global_atomic_add_f32 (no
// compare-and-swap loop), into a g_table that the CALLER zeroed; the order in which the adds of colliding rows arrive changes its last
// bits from run to run.  DESIGN.md records the measured rate and the reproducible alternative (store pass + per-destination sum).
//
// Memory safety does not depend on values: every row is reduced % size_l, every level's offset and size is checked on the host against
// P before anything is launched, and the float-to-integer conversion only ever sees a finite value below 2^30 in magnitude.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gip_model.h"

#define HG_THREADS 256
#define HG_MAX_LEVELS 32
#define HG_MAX_LOG2_SIZE 24

// the level table, by value in the kernel arguments: a level is uniform per workgroup (or per loop trip), so these are scalar loads
struct HashLevels {
  float scale[HG_MAX_LEVELS];
  uint32_t res[HG_MAX_LEVELS];
  uint32_t size[HG_MAX_LEVELS];
  uint32_t hashed[HG_MAX_LEVELS];
  uint64_t offset[HG_MAX_LEVELS];
};

// F floats moved as one access of 4 F bytes (two of 16 for F = 8)
template <int F> struct alignas(F >= 4 ? 16 : 4 * F) HashRow { float v[F]; };

// a point's cell on one level: the corner (cx, cy, cz) as uint32 and the fractions; false when the point has no cell there
__device__ __forceinline__ bool hg_cell(const float* __restrict__ x, int64_t n, float scale, uint32_t c[3], float fr[3]) {
  bool ok = true;
  float cell[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const float pos = x[3 * n + k] * scale + 0.5f;
    ok = ok && fabsf(pos) < 0x1p30f;                    // false for a NaN and for an infinity too
    cell[k] = floorf(pos);
    fr[k] = pos - cell[k];
  }
#pragma unroll
  for (int k = 0; k < 3; k++) c[k] = (uint32_t)(int32_t)(ok ? cell[k] : 0.f);
  return ok;
}

__device__ __forceinline__ uint32_t hg_row(uint32_t cx, uint32_t cy, uint32_t cz, uint32_t res, uint32_t size, bool hashed) {
  const uint32_t i = hashed ? (cx ^ (cy * 2654435761u) ^ (cz * 805459861u)) : (cx + cy * res + cz * (res * res));
  return (size & (size - 1u)) == 0u ? (i & (size - 1u)) : (i % size);          // the same value; size is uniform, and never 0
}

__device__ __forceinline__ float hg_weight(const float fr[3], int k) {
  return ((k & 1) ? fr[0] : 1.f - fr[0]) * ((k & 2) ? fr[1] : 1.f - fr[1]) * ((k & 4) ? fr[2] : 1.f - fr[2]);
}

template <int F>
__global__ void __launch_bounds__(HG_THREADS)
hashgrid_forward_kernel(const float* __restrict__ x, const float* __restrict__ table, HashLevels lv, int64_t N, int L, float* __restrict__ enc) {
  const int l = blockIdx.y;
  const int64_t n = (int64_t)blockIdx.x * HG_THREADS + threadIdx.x;
  if (n >= N) return;
  const uint32_t res = lv.res[l], size = lv.size[l];
  const bool hashed = lv.hashed[l] != 0;
  const float* __restrict__ slice = table + lv.offset[l] * F;
  HashRow<F> acc;
#pragma unroll
  for (int f = 0; f < F; f++) acc.v[f] = 0.f;
  uint32_t c[3];
  float fr[3];
  if (hg_cell(x, n, lv.scale[l], c, fr)) {
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const uint32_t row = hg_row(c[0] + (k & 1), c[1] + ((k >> 1) & 1), c[2] + (k >> 2), res, size, hashed);
      const HashRow<F> t = *(const HashRow<F>*)(slice + (size_t)row * F);
      const float w = hg_weight(fr, k);
#pragma unroll
      for (int f = 0; f < F; f++) acc.v[f] += w * t.v[f];
    }
  }
  *(HashRow<F>*)(enc + ((size_t)n * L + l) * F) = acc;
}

template <int F>
__global__ void __launch_bounds__(HG_THREADS)
hashgrid_backward_table_kernel(const float* __restrict__ x, const float* __restrict__ g_enc, HashLevels lv, int64_t N, int L,
                               float* __restrict__ g_table) {
  const int l = blockIdx.y;
  const int64_t n = (int64_t)blockIdx.x * HG_THREADS + threadIdx.x;
  if (n >= N) return;
  const uint32_t res = lv.res[l], size = lv.size[l];
  const bool hashed = lv.hashed[l] != 0;
  float* __restrict__ slice = g_table + lv.offset[l] * F;
  uint32_t c[3];
  float fr[3];
  if (!hg_cell(x, n, lv.scale[l], c, fr)) return;
  const HashRow<F> g = *(const HashRow<F>*)(g_enc + ((size_t)n * L + l) * F);
  bool any = false;
#pragma unroll
  for (int f = 0; f < F; f++) any = any || g.v[f] != 0.f;
  if (!any) return;                                     // a masked level: adding zeros changes nothing
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const uint32_t row = hg_row(c[0] + (k & 1), c[1] + ((k >> 1) & 1), c[2] + (k >> 2), res, size, hashed);
    const float w = hg_weight(fr, k);
#pragma unroll
    for (int f = 0; f < F; f++) atomicAdd(slice + (size_t)row * F + f, w * g.v[f]);
  }
}

template <int F>
__global__ void __launch_bounds__(HG_THREADS)
hashgrid_backward_input_kernel(const float* __restrict__ x, const float* __restrict__ table, const float* __restrict__ g_enc, HashLevels lv,
                               int64_t N, int L, float* __restrict__ g_x) {
  const int64_t n = (int64_t)blockIdx.x * HG_THREADS + threadIdx.x;
  if (n >= N) return;
  float gx = 0.f, gy = 0.f, gz = 0.f;
  for (int l = 0; l < L; l++) {
    const uint32_t res = lv.res[l], size = lv.size[l];
    const bool hashed = lv.hashed[l] != 0;
    const float scale = lv.scale[l];
    const float* __restrict__ slice = table + lv.offset[l] * F;
    uint32_t c[3];
    float fr[3];
    if (!hg_cell(x, n, scale, c, fr)) continue;
    const HashRow<F> g = *(const HashRow<F>*)(g_enc + ((size_t)n * L + l) * F);
    float d[8];                                         // d_k = g . table row of corner k
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const uint32_t row = hg_row(c[0] + (k & 1), c[1] + ((k >> 1) & 1), c[2] + (k >> 2), res, size, hashed);
      const HashRow<F> t = *(const HashRow<F>*)(slice + (size_t)row * F);
      float s = 0.f;
#pragma unroll
      for (int f = 0; f < F; f++) s += g.v[f] * t.v[f];
      d[k] = s;
    }
    const float x0 = 1.f - fr[0], x1 = fr[0], y0 = 1.f - fr[1], y1 = fr[1], z0 = 1.f - fr[2], z1 = fr[2];
    gx += scale * (((y0 * z0) * (d[1] - d[0]) + (y1 * z0) * (d[3] - d[2])) + ((y0 * z1) * (d[5] - d[4]) + (y1 * z1) * (d[7] - d[6])));
    gy += scale * (((x0 * z0) * (d[2] - d[0]) + (x1 * z0) * (d[3] - d[1])) + ((x0 * z1) * (d[6] - d[4]) + (x1 * z1) * (d[7] - d[5])));
    gz += scale * (((x0 * y0) * (d[4] - d[0]) + (x1 * y0) * (d[5] - d[1])) + ((x0 * y1) * (d[6] - d[2]) + (x1 * y1) * (d[7] - d[3])));
  }
  g_x[3 * n] = gx;
  g_x[3 * n + 1] = gy;
  g_x[3 * n + 2] = gz;
}

// ------------------------------------------------------------------------------------------------------------------------ host
// The limits of the header and the level table against P; fills *lv.  false: the caller returns the bad-argument status.
static bool hg_config(const float* level_scale, const int32_t* level_res, const int32_t* level_size, const int64_t* level_offset,
                      const int32_t* level_hashed, int64_t N, int32_t L, int32_t F, int64_t P, HashLevels* lv) {
  if (L < 1 || L > HG_MAX_LEVELS || !(F == 1 || F == 2 || F == 4 || F == 8) || N < 0 || P < 1) return false;
  if ((uint64_t)N * (uint64_t)L * (uint64_t)F * 4u > (uint64_t)UINT32_MAX) return false;          // N < 2^30, so the product cannot wrap
  if (!level_scale || !level_res || !level_size || !level_offset || !level_hashed) return false;
  int64_t sum = 0;
  for (int l = 0; l < L; l++) {
    if (!isfinite(level_scale[l]) || level_res[l] < 1 || level_size[l] < 1 || level_size[l] > (1 << HG_MAX_LOG2_SIZE)) return false;
    if (level_offset[l] != sum) return false;
    sum += level_size[l];
    if (sum > P) return false;
    lv->scale[l] = level_scale[l];
    lv->res[l] = (uint32_t)level_res[l];
    lv->size[l] = (uint32_t)level_size[l];
    lv->hashed[l] = level_hashed[l] ? 1u : 0u;
    lv->offset[l] = (uint64_t)level_offset[l];
  }
  return sum == P;
}

// a row of F floats is moved in accesses of min(4 F, 16) bytes
static bool hg_aligned(const void* p, int32_t F) { return ((uintptr_t)p & (uintptr_t)((F >= 4 ? 16 : 4 * F) - 1)) == 0; }

static dim3 hg_grid(int64_t N, int32_t levels) { return dim3((unsigned)((N + HG_THREADS - 1) / HG_THREADS), (unsigned)levels); }

static int hg_done(void) { return hipGetLastError() == hipSuccess ? 0 : 3; }

#define HG_DISPATCH(F, kernel, grid, stream, ...)                                                               \
  switch (F) {                                                                                                 \
    case 1: hipLaunchKernelGGL(kernel<1>, grid, dim3(HG_THREADS), 0, (hipStream_t)(stream), __VA_ARGS__); break; \
    case 2: hipLaunchKernelGGL(kernel<2>, grid, dim3(HG_THREADS), 0, (hipStream_t)(stream), __VA_ARGS__); break; \
    case 4: hipLaunchKernelGGL(kernel<4>, grid, dim3(HG_THREADS), 0, (hipStream_t)(stream), __VA_ARGS__); break; \
    default: hipLaunchKernelGGL(kernel<8>, grid, dim3(HG_THREADS), 0, (hipStream_t)(stream), __VA_ARGS__); break; \
  }

extern "C" int gip_hashgrid_forward(const float* x, const float* table, const float* level_scale, const int32_t* level_res,
                                    const int32_t* level_size, const int64_t* level_offset, const int32_t* level_hashed, int64_t N, int32_t L,
                                    int32_t F, int64_t P, float* enc, void* stream) {
  HashLevels lv;
  if (!hg_config(level_scale, level_res, level_size, level_offset, level_hashed, N, L, F, P, &lv)) return 1;
  if (N == 0) return 0;
  if (!x || !table || !enc || !hg_aligned(table, F) || !hg_aligned(enc, F)) return 1;
  HG_DISPATCH(F, hashgrid_forward_kernel, hg_grid(N, L), stream, x, table, lv, N, (int)L, enc);
  return hg_done();
}

extern "C" int gip_hashgrid_backward_input(const float* x, const float* table, const float* g_enc, const float* level_scale,
                                           const int32_t* level_res, const int32_t* level_size, const int64_t* level_offset,
                                           const int32_t* level_hashed, int64_t N, int32_t L, int32_t F, int64_t P, float* g_x, void* stream) {
  HashLevels lv;
  if (!hg_config(level_scale, level_res, level_size, level_offset, level_hashed, N, L, F, P, &lv)) return 1;
  if (N == 0) return 0;
  if (!x || !table || !g_enc || !g_x || !hg_aligned(table, F) || !hg_aligned(g_enc, F)) return 1;
  HG_DISPATCH(F, hashgrid_backward_input_kernel, hg_grid(N, 1), stream, x, table, g_enc, lv, N, (int)L, g_x);
  return hg_done();
}

extern "C" int gip_hashgrid_backward_table(const float* x, const float* g_enc, const float* level_scale, const int32_t* level_res,
                                           const int32_t* level_size, const int64_t* level_offset, const int32_t* level_hashed, int64_t N,
                                           int32_t L, int32_t F, int64_t P, float* g_table, void* stream) {
  HashLevels lv;
  if (!hg_config(level_scale, level_res, level_size, level_offset, level_hashed, N, L, F, P, &lv)) return 1;
  if (N == 0) return 0;
  if (!x || !g_enc || !g_table || !hg_aligned(g_enc, F)) return 1;
  HG_DISPATCH(F, hashgrid_backward_table_kernel, hg_grid(N, L), stream, x, g_enc, lv, N, (int)L, g_table);
  return hg_done();
}
