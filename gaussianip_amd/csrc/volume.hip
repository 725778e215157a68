// volume.hip — volume rendering of a density field: marching rays through an occupancy grid, and compositing along them with
// gradients.  It is what the reference's nerf-volume-renderer (threestudio/models/renderers/nerf_volume_renderer.py) gets from nerfacc:
// OccGridEstimator.sampling (:84, :96), render_weight_from_density (:150) and accumulate_along_rays (:158-170).  nerfacc is CUDA-only, so
// the definition below is the project's own; it has not been compared with nerfacc's output.
// Linked into libgip_model.so; gaussianip_amd/utils/volume.py is the host side.
//
// Definition.  Everything is float32 with every operation rounded on its own (-ffp-contract=off); min(a, b) is `b < a ? b : a` and
// max(a, b) is `b > a ? b : a`, so a NaN on the right is dropped and one on the left is kept, the same in every restatement.
//
// Marching.  rays_o, rays_d [R, 3]; occ [G, G, G] uint8 in the index order [ix, iy, iz], 1 <= G <= 256; the box (lo, hi) and the
// per-axis scale = G / (hi - lo), computed in float32 ON THE HOST and passed by value; dt > 0, near, far; jitter [R] in [0, 1), NULL
// meaning 0; K_cap, the most candidate steps of one ray.  Per ray:
//   a ray with a non-finite origin or direction, or an all-zero direction, has no samples;
//   an axis with d == 0 contributes no bounds, and the ray misses unless lo <= o <= hi on that axis;
//   any other axis: inv = 1 / d, ta = (lo - o) * inv, tb = (hi - o) * inv; t_near = max over these axes, in the order x, y, z and
//     starting from near, of min(ta, tb); t_far = min over them, starting from far, of max(ta, tb);
//   the ray misses unless t_near < t_far;
//   candidate k = 0 .. K_cap - 1: ts = t_near + ((float)k + jitter) * dt, which exists while ts < t_far; te = min(ts + dt, t_far),
//     tm = (ts + te) * 0.5, p = o + d * tm per axis;
//   its cell per axis: f = floorf((p - lo) * scale), c = f >= G - 1 ? G - 1 : (f > 0 ? (int)f : 0), which is
//     clamp((int)floorf(.), 0, G - 1) wherever that conversion is defined and 0 for a NaN; the candidate is kept iff occ[cx, cy, cz] != 0.
// ts comes from k by formula, not by accumulation, and it does not decrease with k: candidates are independent, and the first one that
// does not exist ends the ray.  A ray's kept candidates are its samples, in the order of k, that is of t.
//
// Weights (render_weight_from_density).  t_starts, t_ends, sigmas [M]; the samples of ray r are the row [offsets[r], offsets[r + 1]) of
// the CSR offsets [R + 1], clamped to [0, M]:
//   x_i = sigma_i * (te_i - ts_i),  trans_i = expf(-(sum of x_j over the samples j < i of the ray)),  alpha_i = 1 - expf(-x_i),
//   w_i = trans_i * alpha_i.
//   The sum before sample i of the trip that starts at sample b (b - row start a multiple of 64) is carry + e_i: carry is the sum of the
//   earlier trips' totals in trip order, a trip's total is its last lane's inclusive scan, and the scan is the doubling one: s = x; for
//   d = 1, 2, .. 32: s_lane += s_(lane - d) for lane >= d; e_i is s of the lane before (0 for the first).  The order is fixed.
//   Backward: g_sigma_i = (te_i - ts_i) * (g_w_i * trans_i * (1 - alpha_i) - sum over the samples k > i of the ray of g_w_k * w_k), the
//   trips walked from the last to the first with the mirrored scan.  No gradient to t_starts / t_ends.
// Accumulate (accumulate_along_rays).  out[r, c] = sum over the samples i of ray r of w_i * v[i, c], C = 1 .. 16 channels; values NULL
//   means v = 1 and C = 1; a ray without samples gives 0.  A lane sums its samples (row start + lane, + 64, ...) in that order, then the
//   64 lanes are summed by the xor butterfly 32, 16, .. 1.  Backward, per sample: g_w_i = sum_c g_out[ray_i, c] * v[i, c] in the order
//   of c, g_v[i, c] = w_i * g_out[ray_i, c]; a ray_indices entry outside [0, R) gives zeros.
//
// Kernels (wave64).  Every kernel but the last gives one WAVE to a ray, four rays to a workgroup, and walks the ray 64 candidates or
// samples per trip: the march with a ballot and a population count (a kept candidate's row is the row start + the kept so far + the
// kept lanes below it), the weights with a wave-wide scan and the trip's total carried in a register, the accumulate with per-lane
// partial sums.  volume_accumulate_backward_kernel takes one lane per sample.  Nothing here uses an atomic: every output is bitwise
// equal from run to run.  The count and the emit launch of the march run the same function (vol_march), so they cannot disagree.
//
// Memory safety does not depend on values: a cell index is clamped per axis to [0, G - 1] through comparisons that a NaN fails, an
// emitted row is compared with M before it is written, a CSR row is clamped to [0, M], and a ray index is compared with R.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gip_model.h"
#include "volume_common.h"

#define VOL_MAX_GRID 256

// the box and the grid, by value in the kernel arguments: uniform, so these are scalar loads
struct VolGrid {
  float lo[3], hi[3], scale[3];
  int G;
};

// [t_near, t_far) of a ray in the box; false when the ray has no samples
__device__ __forceinline__ bool vol_span(const float o[3], const float d[3], const VolGrid& g, float near, float far, float* t_near, float* t_far) {
  bool ok = true, any = false;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    ok = ok && fabsf(o[a]) < INFINITY && fabsf(d[a]) < INFINITY;       // false for a NaN too
    any = any || d[a] != 0.f;
  }
  if (!(ok && any)) return false;
  float tn = near, tf = far;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    if (d[a] == 0.f) {
      if (!(g.lo[a] <= o[a] && o[a] <= g.hi[a])) return false;
    } else {
      const float inv = 1.f / d[a];
      const float ta = (g.lo[a] - o[a]) * inv, tb = (g.hi[a] - o[a]) * inv;
      tn = vol_max(tn, vol_min(ta, tb));
      tf = vol_min(tf, vol_max(ta, tb));
    }
  }
  *t_near = tn;
  *t_far = tf;
  return tn < tf;
}

__device__ __forceinline__ int vol_cell(float p, float lo, float scale, int G) {
  const float f = floorf((p - lo) * scale);
  return f >= (float)(G - 1) ? G - 1 : (f > 0.f ? (int)f : 0);
}

// One wave marches ray r.  EMIT false: returns the number of kept candidates.  EMIT true: also writes them from row `base` on.
template <bool EMIT>
__device__ __forceinline__ int vol_march(const float* __restrict__ rays_o, const float* __restrict__ rays_d, const uint8_t* __restrict__ occ,
                                         const float* __restrict__ jitter, const VolGrid& g, float dt, float near, float far, int K_cap,
                                         int64_t r, int lane, int64_t base, int64_t M, int32_t* __restrict__ ray_indices,
                                         float* __restrict__ t_starts, float* __restrict__ t_ends) {
  const float o[3] = {rays_o[3 * r], rays_o[3 * r + 1], rays_o[3 * r + 2]};
  const float d[3] = {rays_d[3 * r], rays_d[3 * r + 1], rays_d[3 * r + 2]};
  float t_near, t_far;
  if (!vol_span(o, d, g, near, far, &t_near, &t_far)) return 0;          // uniform: the whole wave reads one ray
  const float jit = jitter ? jitter[r] : 0.f;
  int kept_before = 0;
  for (int k0 = 0; k0 < K_cap; k0 += 64) {
    const int k = k0 + lane;
    const float ts = t_near + ((float)k + jit) * dt;
    const bool exists = k < K_cap && ts < t_far;
    const unsigned long long there = __ballot(exists);
    if (!(there & 1ull)) break;                                           // the trip's first candidate does not exist: nor does any later one
    const float te = vol_min(ts + dt, t_far);
    bool kept = false;
    if (exists) {
      const float tm = (ts + te) * 0.5f;
      const int cx = vol_cell(o[0] + d[0] * tm, g.lo[0], g.scale[0], g.G);
      const int cy = vol_cell(o[1] + d[1] * tm, g.lo[1], g.scale[1], g.G);
      const int cz = vol_cell(o[2] + d[2] * tm, g.lo[2], g.scale[2], g.G);
      kept = occ[(cx * g.G + cy) * g.G + cz] != 0;
    }
    const unsigned long long keep = __ballot(kept);
    if (EMIT && kept) {
      const int64_t row = base + kept_before + __popcll(keep & ((1ull << lane) - 1ull));
      if (row >= 0 && row < M) {
        ray_indices[row] = (int32_t)r;
        t_starts[row] = ts;
        t_ends[row] = te;
      }
    }
    kept_before += __popcll(keep);
  }
  return kept_before;
}

__global__ void __launch_bounds__(MESH_THREADS)
volume_march_count_kernel(const float* __restrict__ rays_o, const float* __restrict__ rays_d, const uint8_t* __restrict__ occ,
                          const float* __restrict__ jitter, VolGrid g, float dt, float near, float far, int K_cap, int64_t R,
                          int32_t* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * VOL_RAYS_PER_BLOCK + (threadIdx.x >> 6);
  if (r >= R) return;
  const int n = vol_march<false>(rays_o, rays_d, occ, jitter, g, dt, near, far, K_cap, r, lane, 0, 0, nullptr, nullptr, nullptr);
  if (lane == 0) counts[r] = n;
}

__global__ void __launch_bounds__(MESH_THREADS)
volume_march_emit_kernel(const float* __restrict__ rays_o, const float* __restrict__ rays_d, const uint8_t* __restrict__ occ,
                         const float* __restrict__ jitter, VolGrid g, float dt, float near, float far, int K_cap, int64_t R,
                         const int32_t* __restrict__ offsets, int64_t M, int32_t* __restrict__ ray_indices, float* __restrict__ t_starts,
                         float* __restrict__ t_ends) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * VOL_RAYS_PER_BLOCK + (threadIdx.x >> 6);
  if (r >= R) return;
  vol_march<true>(rays_o, rays_d, occ, jitter, g, dt, near, far, K_cap, r, lane, offsets[r], M, ray_indices, t_starts, t_ends);
}

__global__ void __launch_bounds__(MESH_THREADS)
volume_weights_forward_kernel(const float* __restrict__ t_starts, const float* __restrict__ t_ends, const float* __restrict__ sigmas,
                              const int32_t* __restrict__ offsets, int64_t R, int64_t M, float* __restrict__ weights,
                              float* __restrict__ trans, float* __restrict__ alphas) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * VOL_RAYS_PER_BLOCK + (threadIdx.x >> 6);
  if (r >= R) return;
  int64_t lo, hi;
  mesh_row(offsets, r, M, &lo, &hi);
  float carry = 0.f;
  for (int64_t b = lo; b < hi; b += 64) {
    const int64_t i = b + lane;
    const float x = i < hi ? sigmas[i] * (t_ends[i] - t_starts[i]) : 0.f;
    const float s = vol_scan<true>(x, lane);
    const float before = __shfl_up(s, 1, 64);
    const float total = __shfl(s, 63, 64);
    if (i < hi) {
      const float T = expf(-(carry + (lane ? before : 0.f)));
      const float a = 1.f - expf(-x);
      trans[i] = T;
      alphas[i] = a;
      weights[i] = T * a;
    }
    carry += total;
  }
}

__global__ void __launch_bounds__(MESH_THREADS)
volume_weights_backward_kernel(const float* __restrict__ t_starts, const float* __restrict__ t_ends, const float* __restrict__ g_weights,
                               const float* __restrict__ weights, const float* __restrict__ trans, const float* __restrict__ alphas,
                               const int32_t* __restrict__ offsets, int64_t R, int64_t M, float* __restrict__ g_sigmas) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * VOL_RAYS_PER_BLOCK + (threadIdx.x >> 6);
  if (r >= R) return;
  int64_t lo, hi;
  mesh_row(offsets, r, M, &lo, &hi);
  if (hi <= lo) return;
  float carry = 0.f;
  for (int64_t b = lo + (hi - lo - 1) / 64 * 64; b >= lo; b -= 64) {
    const int64_t i = b + lane;
    const float gw = i < hi ? g_weights[i] : 0.f;
    const float y = i < hi ? gw * weights[i] : 0.f;
    const float s = vol_scan<false>(y, lane);
    const float after = __shfl_down(s, 1, 64);
    const float total = __shfl(s, 0, 64);
    if (i < hi) g_sigmas[i] = (t_ends[i] - t_starts[i]) * (gw * trans[i] * (1.f - alphas[i]) - (carry + (lane < 63 ? after : 0.f)));
    carry += total;
  }
}

__global__ void __launch_bounds__(MESH_THREADS)
volume_accumulate_forward_kernel(const float* __restrict__ weights, const float* __restrict__ values, const int32_t* __restrict__ offsets,
                                 int64_t R, int64_t M, int C, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * VOL_RAYS_PER_BLOCK + (threadIdx.x >> 6);
  if (r >= R) return;
  int64_t lo, hi;
  mesh_row(offsets, r, M, &lo, &hi);
  float acc[VOL_MAX_CHANNELS];
#pragma unroll
  for (int c = 0; c < VOL_MAX_CHANNELS; c++) acc[c] = 0.f;
  for (int64_t i = lo + lane; i < hi; i += 64) {
    const float w = weights[i];
    if (values) {
#pragma unroll
      for (int c = 0; c < VOL_MAX_CHANNELS; c++)
        if (c < C) acc[c] += w * values[i * C + c];                      // C is uniform: a scalar branch, and acc stays in registers
    } else {
      acc[0] += w;
    }
  }
#pragma unroll
  for (int c = 0; c < VOL_MAX_CHANNELS; c++) {
    if (c < C) {
      const float v = vol_wave_sum(acc[c]);
      if (lane == 0) out[r * C + c] = v;
    }
  }
}

__global__ void __launch_bounds__(MESH_THREADS)
volume_accumulate_backward_kernel(const float* __restrict__ weights, const float* __restrict__ values, const int32_t* __restrict__ ray_indices,
                                  const float* __restrict__ g_out, int64_t R, int64_t M, int C, float* __restrict__ g_weights,
                                  float* __restrict__ g_values) {
  const int64_t i = (int64_t)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (i >= M) return;
  const int64_t r = ray_indices[i];
  const bool ok = (uint64_t)r < (uint64_t)R;
  const float w = weights[i];
  float gw = 0.f;
  for (int c = 0; c < C; c++) {
    const float g = ok ? g_out[r * C + c] : 0.f;
    gw += values ? g * values[i * C + c] : g;
    if (g_values) g_values[i * C + c] = w * g;
  }
  if (g_weights) g_weights[i] = gw;
}

// ------------------------------------------------------------------------------------------------------------------------ host
// The march's arguments; fills *g.  false: the caller returns the bad-argument status.
static bool vol_march_config(int64_t R, int32_t G, const float box[9], float dt, float near, float far, int32_t K_cap, VolGrid* g) {
  if (R < 0 || R > INT32_MAX / 64 || G < 1 || G > VOL_MAX_GRID || K_cap < 1) return false;
  if (R * (int64_t)K_cap > (int64_t)INT32_MAX) return false;                // R K_cap >= 2^31: a row could not be an int32
  if (!(dt > 0.f) || !isfinite(dt) || isnan(near) || isnan(far)) return false;
  for (int a = 0; a < 3; a++) {
    g->lo[a] = box[a];
    g->hi[a] = box[3 + a];
    g->scale[a] = box[6 + a];
    if (!(isfinite(box[a]) && isfinite(box[3 + a]) && box[a] < box[3 + a] && isfinite(box[6 + a]) && box[6 + a] > 0.f)) return false;
  }
  g->G = G;
  return true;
}

#define VOL_BOX_PARAMS float lo_x, float lo_y, float lo_z, float hi_x, float hi_y, float hi_z, float scale_x, float scale_y, float scale_z

extern "C" int gip_volume_march_count(const float* rays_o, const float* rays_d, const uint8_t* occ, const float* jitter, int64_t R, int32_t G,
                                      VOL_BOX_PARAMS, float dt, float near, float far, int32_t K_cap, int32_t* counts, void* stream) {
  VolGrid g;
  const float box[9] = {lo_x, lo_y, lo_z, hi_x, hi_y, hi_z, scale_x, scale_y, scale_z};
  if (!vol_march_config(R, G, box, dt, near, far, K_cap, &g)) return 1;
  if (R == 0) return 0;
  if (!rays_o || !rays_d || !occ || !counts) return 1;
  MESH_LAUNCH(volume_march_count_kernel, vol_ray_blocks(R), stream, rays_o, rays_d, occ, jitter, g, dt, near, far, (int)K_cap, R, counts);
  return mesh_done();
}

extern "C" int gip_volume_march_emit(const float* rays_o, const float* rays_d, const uint8_t* occ, const float* jitter, int64_t R, int32_t G,
                                     VOL_BOX_PARAMS, float dt, float near, float far, int32_t K_cap, const int32_t* offsets, int64_t M,
                                     int32_t* ray_indices, float* t_starts, float* t_ends, void* stream) {
  VolGrid g;
  const float box[9] = {lo_x, lo_y, lo_z, hi_x, hi_y, hi_z, scale_x, scale_y, scale_z};
  if (!vol_march_config(R, G, box, dt, near, far, K_cap, &g) || !mesh_count_ok(M)) return 1;
  if (R == 0 || M == 0) return 0;
  if (!rays_o || !rays_d || !occ || !offsets || !ray_indices || !t_starts || !t_ends) return 1;
  MESH_LAUNCH(volume_march_emit_kernel, vol_ray_blocks(R), stream, rays_o, rays_d, occ, jitter, g, dt, near, far, (int)K_cap, R, offsets, M,
              ray_indices, t_starts, t_ends);
  return mesh_done();
}

extern "C" int gip_volume_weights_forward(const float* t_starts, const float* t_ends, const float* sigmas, const int32_t* offsets, int64_t R,
                                          int64_t M, float* weights, float* trans, float* alphas, void* stream) {
  if (!vol_rows_ok(R, M)) return 1;
  if (R == 0 || M == 0) return 0;
  if (!t_starts || !t_ends || !sigmas || !offsets || !weights || !trans || !alphas) return 1;
  MESH_LAUNCH(volume_weights_forward_kernel, vol_ray_blocks(R), stream, t_starts, t_ends, sigmas, offsets, R, M, weights, trans, alphas);
  return mesh_done();
}

extern "C" int gip_volume_weights_backward(const float* t_starts, const float* t_ends, const float* g_weights, const float* weights,
                                           const float* trans, const float* alphas, const int32_t* offsets, int64_t R, int64_t M,
                                           float* g_sigmas, void* stream) {
  if (!vol_rows_ok(R, M)) return 1;
  if (R == 0 || M == 0) return 0;
  if (!t_starts || !t_ends || !g_weights || !weights || !trans || !alphas || !offsets || !g_sigmas) return 1;
  MESH_LAUNCH(volume_weights_backward_kernel, vol_ray_blocks(R), stream, t_starts, t_ends, g_weights, weights, trans, alphas, offsets, R, M,
              g_sigmas);
  return mesh_done();
}

extern "C" int gip_volume_accumulate_forward(const float* weights, const float* values, const int32_t* offsets, int64_t R, int64_t M, int32_t C,
                                             float* out, void* stream) {
  if (!vol_rows_ok(R, M) || C < 1 || C > VOL_MAX_CHANNELS || (!values && C != 1) || M * (int64_t)C > (int64_t)INT32_MAX) return 1;
  if (R == 0) return 0;
  if (!offsets || !out || (M > 0 && !weights)) return 1;
  MESH_LAUNCH(volume_accumulate_forward_kernel, vol_ray_blocks(R), stream, weights, values, offsets, R, M, (int)C, out);
  return mesh_done();
}

extern "C" int gip_volume_accumulate_backward(const float* weights, const float* values, const int32_t* ray_indices, const float* g_out,
                                              int64_t R, int64_t M, int32_t C, float* g_weights, float* g_values, void* stream) {
  if (!vol_rows_ok(R, M) || C < 1 || C > VOL_MAX_CHANNELS || (!values && C != 1) || M * (int64_t)C > (int64_t)INT32_MAX) return 1;
  if (M == 0) return 0;
  if (!weights || !ray_indices || (R > 0 && !g_out) || (!g_weights && !g_values)) return 1;
  MESH_LAUNCH(volume_accumulate_backward_kernel, mesh_blocks(M), stream, weights, values, ray_indices, g_out, R, M, (int)C, g_weights, g_values);
  return mesh_done();
}
