// volume_sdf.hip — NeuS volume rendering of a signed-distance field: alpha from the SDF, weights from alpha and compositing along the
// ray, fused into one forward and one backward launch, with the two primitives (weights from alpha) beside them.  It is what the
// reference's neus-volume-renderer (threestudio/models/renderers/neus_volume_renderer.py) gets from its get_alpha (:72-96), from
// nerfacc.render_weight_from_alpha (:216) and from nerfacc.accumulate_along_rays (:222-230, :262).  nerfacc is CUDA-only, so the
// definition below is the project's own; it has not been compared with nerfacc's output.
// Linked into libgip_model.so; gaussianip_amd/utils/sdf_volume.py is the host side.
//
// Definition.  Everything is float32 with every operation rounded on its own (-ffp-contract=off); eps = 1e-5; sigmoid(x) =
// 1 / (1 + expf(-x)); relu(x) = max(0, x) and clip(q) = min(max(q, 0), 1) with volume_common.h's min and max.  The samples of ray r
// are the row [offsets[r], offsets[r + 1]) of the CSR offsets [R + 1], clamped to [0, M].  beta = *inv_std, one float on the device, read by pointer (no host read; uniform, a scalar load);
// rho = cos_anneal_ratio by value; d_r = rays_d[r], indexed by the ray (uniform), not gathered per sample.
//
// Alpha (get_alpha with use_volsdf off).  Per sample i of ray r, with s = sdf[i], n_i = normals[i], delta = te_i - ts_i:
//   t = d_r.x n_i.x + d_r.y n_i.y + d_r.z n_i.z,  ic = -(relu(-0.5 t + 0.5) (1 - rho) + relu(-t) rho);  normals NULL: ic = -1, the
//   reference's alpha_fn / occ_eval_fn form, where delta is the step;
//   h = ic delta 0.5,  prev = s - h,  next = s + h,  c = sigmoid(prev beta),  m = sigmoid(next beta),
//   q = (c - m + eps) / (c + eps),  alpha = clip(q)   (a NaN stays a NaN).
// Weights (render_weight_from_alpha).  trans_i = the product of (1 - alpha_j) over the samples j < i of the ray, w_i = trans_i alpha_i.
//   The product before sample i of the trip that starts at sample b (b - row start a multiple of 64) is carry * e_i: carry is the
//   product of the earlier trips' totals in trip order (1 at the start), a trip's total is its last lane's inclusive scan (lanes past
//   the row's end count as 1), and the scan is the doubling one: p = 1 - alpha; for d = 1, 2, .. 32: p_lane *= p_(lane - d) for
//   lane >= d; e_i is p of the lane before (1 for the first).  The order is fixed.
// Accumulate.  out[r, 0] = sum of w_i (opacity), out[r, 1] = sum of w_i tm_i with tm = (ts + te) 0.5 (depth), out[r, 2 + k] = sum of
//   w_i v[i, k] for k < C, 0 <= C <= 16; values NULL means C = 0.  A lane sums its samples (row start + lane, + 64, ...) in that order,
//   then the 64 lanes are summed by the xor butterfly 32, 16, .. 1.  A ray without samples gives zeros.
//
// Backward.  g_w_i = g_weights_i (0 when NULL) + g_out[r, 0] + g_out[r, 1] tm_i + sum over k of g_out[r, 2 + k] v[i, k], in that
//   order; g_v[i, k] = w_i g_out[r, 2 + k].
//   Weights, WITHOUT A DIVISION: U_last = 0, U_i = alpha_(i+1) g_w_(i+1) + (1 - alpha_(i+1)) U_(i+1), g_alpha_i = trans_i (g_w_i - U_i).
//   The textbook form divides the later samples' sum by 1 - alpha_i, which is 0 / 0 at alpha_i == 1, the normal state of a sample
//   behind the surface.  Sample i stands for the affine map f_i(u) = alpha_i g_w_i + (1 - alpha_i) u (lanes past the row's end: the
//   identity); the trips are walked from the last to the first, a trip composes its maps towards lower lanes by the doubling scan
//   (mul, add)_lane = (mul_lane mul_(lane + d), add_lane + mul_lane add_(lane + d)) for lane + d < 64, d = 1, 2, .. 32; U_i is the
//   scanned map of lane + 1 applied to carry (carry itself for lane 63), carry is U after the trip's last sample (0 at the start), and
//   the next carry is lane 0's scanned map applied to it.
//   Alpha: g_q = g_alpha iff 0 <= q <= 1 (torch.clip's rule), else 0;  g_xp = g_q m / (c + eps)^2 c (1 - c),
//   g_xn = -g_q / (c + eps) m (1 - m),  g_s = beta (g_xp + g_xn),  g_beta += g_xp prev + g_xn next,  g_ic = beta (g_xn - g_xp) delta 0.5,
//   dic/dt = 0.5 (1 - rho) [-0.5 t + 0.5 > 0] + rho [t < 0],  g_n = g_ic dic/dt d_r.  No gradient to the rays or the samples.
//   g_beta is summed per ray like an output (lane partials in trip order, here from the last trip to the first, then the butterfly)
//   into g_inv_std_rays[R]; the host adds those.
//
// Kernels (wave64): one WAVE per ray, four rays per workgroup, 64 samples per trip, as the density renderer assigns work.  No LDS, no
// atomics, no scratch: every output is bitwise equal from run to run.  The two primitive kernels and the fused pair run the same two
// device functions for the product scan and for the affine scan.
//
// Memory safety does not depend on values: a CSR row is clamped to [0, M], the ray is compared with R, C with 16.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gip_model.h"
#include "volume_common.h"

#define SDF_EPS 1e-5f

// trans of this lane's sample: carry x the product of (1 - alpha) over the trip's lanes below; carry becomes the product through the trip
__device__ __forceinline__ float sdf_product_scan(float alpha, bool live, int lane, float* carry) {
  float p = live ? 1.f - alpha : 1.f;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const float y = __shfl_up(p, d, 64);
    if (lane >= d) p *= y;
  }
  const float before = __shfl_up(p, 1, 64);
  const float total = __shfl(p, 63, 64);
  const float T = *carry * (lane ? before : 1.f);
  *carry = *carry * total;
  return T;
}

// U of this lane's sample from the maps (mul, add) of the trip's lanes above and carry, U after the trip; carry becomes U before it
__device__ __forceinline__ float sdf_affine_scan(float alpha, float g_w, bool live, int lane, float* carry) {
  float mul = live ? 1.f - alpha : 1.f, add = live ? alpha * g_w : 0.f;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const float m2 = __shfl_down(mul, d, 64), a2 = __shfl_down(add, d, 64);
    if (lane + d < 64) {
      add = add + mul * a2;
      mul = mul * m2;
    }
  }
  const float m_up = __shfl_down(mul, 1, 64), a_up = __shfl_down(add, 1, 64);
  const float c = *carry;
  const float U = lane < 63 ? a_up + m_up * c : c;
  *carry = __shfl(add, 0, 64) + __shfl(mul, 0, 64) * c;
  return U;
}

__device__ __forceinline__ float sdf_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// what alpha's forward and backward both need of one sample
struct SdfAlpha {
  float t, prev, next, c, m, q;
};

__device__ __forceinline__ SdfAlpha sdf_alpha(float s, float delta, bool has_n, float nx, float ny, float nz, float dx, float dy, float dz,
                                              float beta, float rho) {
  SdfAlpha a;
  float ic = -1.f;
  a.t = 0.f;
  if (has_n) {
    a.t = dx * nx + dy * ny + dz * nz;
    const float half = -0.5f * a.t + 0.5f, neg = -a.t;
    ic = -(vol_max(0.f, half) * (1.f - rho) + vol_max(0.f, neg) * rho);
  }
  const float h = ic * delta * 0.5f;
  a.prev = s - h;
  a.next = s + h;
  a.c = sdf_sigmoid(a.prev * beta);
  a.m = sdf_sigmoid(a.next * beta);
  a.q = (a.c - a.m + SDF_EPS) / (a.c + SDF_EPS);
  return a;
}

__device__ __forceinline__ float sdf_clip(float q) { return vol_min(vol_max(q, 0.f), 1.f); }

// the ray of this wave as a uniform value, so that what is indexed by it is loaded once per wave; -1 past the last ray
__device__ __forceinline__ int64_t sdf_ray(int64_t R) {
  const int64_t r = (int64_t)blockIdx.x * VOL_RAYS_PER_BLOCK + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  return r < R ? r : -1;
}

__global__ void __launch_bounds__(MESH_THREADS)
volume_alpha_weights_forward_kernel(const float* __restrict__ alphas, const int32_t* __restrict__ offsets, int64_t R, int64_t M,
                                    float* __restrict__ weights, float* __restrict__ trans) {
  const int lane = threadIdx.x & 63;
  const int64_t r = sdf_ray(R);
  if (r < 0) return;
  int64_t lo, hi;
  mesh_row(offsets, r, M, &lo, &hi);
  float carry = 1.f;
  for (int64_t b = lo; b < hi; b += 64) {
    const int64_t i = b + lane;
    const bool live = i < hi;
    const float a = live ? alphas[i] : 0.f;
    const float T = sdf_product_scan(a, live, lane, &carry);
    if (live) {
      trans[i] = T;
      weights[i] = T * a;
    }
  }
}

__global__ void __launch_bounds__(MESH_THREADS)
volume_alpha_weights_backward_kernel(const float* __restrict__ alphas, const float* __restrict__ trans, const float* __restrict__ g_weights,
                                     const int32_t* __restrict__ offsets, int64_t R, int64_t M, float* __restrict__ g_alphas) {
  const int lane = threadIdx.x & 63;
  const int64_t r = sdf_ray(R);
  if (r < 0) return;
  int64_t lo, hi;
  mesh_row(offsets, r, M, &lo, &hi);
  if (hi <= lo) return;
  float carry = 0.f;
  for (int64_t b = lo + (hi - lo - 1) / 64 * 64; b >= lo; b -= 64) {
    const int64_t i = b + lane;
    const bool live = i < hi;
    const float a = live ? alphas[i] : 0.f, gw = live ? g_weights[i] : 0.f;
    const float U = sdf_affine_scan(a, gw, live, lane, &carry);
    if (live) g_alphas[i] = trans[i] * (gw - U);
  }
}

__global__ void __launch_bounds__(MESH_THREADS)
volume_sdf_render_forward_kernel(const float* __restrict__ sdf, const float* __restrict__ normals, const float* __restrict__ rays_d,
                                 const float* __restrict__ t_starts, const float* __restrict__ t_ends, const float* __restrict__ values,
                                 const int32_t* __restrict__ offsets, const float* __restrict__ inv_std, float rho, int64_t R, int64_t M,
                                 int C, float* __restrict__ alphas, float* __restrict__ trans, float* __restrict__ weights,
                                 float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t r = sdf_ray(R);
  if (r < 0) return;
  int64_t lo, hi;
  mesh_row(offsets, r, M, &lo, &hi);
  const float beta = *inv_std;
  const float dx = rays_d[3 * r], dy = rays_d[3 * r + 1], dz = rays_d[3 * r + 2];
  float opacity = 0.f, depth = 0.f, acc[VOL_MAX_CHANNELS];
#pragma unroll
  for (int c = 0; c < VOL_MAX_CHANNELS; c++) acc[c] = 0.f;
  float carry = 1.f;
  for (int64_t b = lo; b < hi; b += 64) {
    const int64_t i = b + lane;
    const bool live = i < hi;
    float a = 0.f, tm = 0.f;
    if (live) {
      const float ts = t_starts[i], te = t_ends[i];
      float nx = 0.f, ny = 0.f, nz = 0.f;
      if (normals) {
        nx = normals[3 * i];
        ny = normals[3 * i + 1];
        nz = normals[3 * i + 2];
      }
      a = sdf_clip(sdf_alpha(sdf[i], te - ts, normals != nullptr, nx, ny, nz, dx, dy, dz, beta, rho).q);
      tm = (ts + te) * 0.5f;
    }
    const float T = sdf_product_scan(a, live, lane, &carry);
    if (live) {
      const float w = T * a;
      alphas[i] = a;
      trans[i] = T;
      weights[i] = w;
      opacity += w;
      depth += w * tm;
#pragma unroll
      for (int c = 0; c < VOL_MAX_CHANNELS; c++)
        if (c < C) acc[c] += w * values[i * C + c];                        // C is uniform: a scalar branch, and acc stays in registers
    }
  }
  const int64_t row = r * (2 + C);
  opacity = vol_wave_sum(opacity);
  depth = vol_wave_sum(depth);
  if (lane == 0) {
    out[row] = opacity;
    out[row + 1] = depth;
  }
#pragma unroll
  for (int c = 0; c < VOL_MAX_CHANNELS; c++) {
    if (c < C) {
      const float v = vol_wave_sum(acc[c]);
      if (lane == 0) out[row + 2 + c] = v;
    }
  }
}

__global__ void __launch_bounds__(MESH_THREADS)
volume_sdf_render_backward_kernel(const float* __restrict__ sdf, const float* __restrict__ normals, const float* __restrict__ rays_d,
                                  const float* __restrict__ t_starts, const float* __restrict__ t_ends, const float* __restrict__ values,
                                  const int32_t* __restrict__ offsets, const float* __restrict__ inv_std, float rho,
                                  const float* __restrict__ alphas, const float* __restrict__ trans, const float* __restrict__ weights,
                                  const float* __restrict__ g_out, const float* __restrict__ g_weights, int64_t R, int64_t M, int C,
                                  float* __restrict__ g_sdf, float* __restrict__ g_normals, float* __restrict__ g_values,
                                  float* __restrict__ g_inv_std_rays) {
  const int lane = threadIdx.x & 63;
  const int64_t r = sdf_ray(R);
  if (r < 0) return;
  int64_t lo, hi;
  mesh_row(offsets, r, M, &lo, &hi);
  if (hi <= lo) {
    if (lane == 0) g_inv_std_rays[r] = 0.f;
    return;
  }
  const float beta = *inv_std;
  const float dx = rays_d[3 * r], dy = rays_d[3 * r + 1], dz = rays_d[3 * r + 2];
  // g_out's row goes through the lane's own copy of the ray: eighteen vector registers, where the uniform index would ask for
  // eighteen scalar ones on top of the twenty-one arguments and spill them
  const int64_t row = ((int64_t)blockIdx.x * VOL_RAYS_PER_BLOCK + (threadIdx.x >> 6)) * (2 + C);
  const float go_opacity = g_out[row], go_depth = g_out[row + 1];
  float go[VOL_MAX_CHANNELS];
#pragma unroll
  for (int c = 0; c < VOL_MAX_CHANNELS; c++) go[c] = c < C ? g_out[row + 2 + c] : 0.f;
  float carry = 0.f, g_beta = 0.f;
  // the row lies in [0, M] and M in 31 bits: the trip's start as an int, which halves the scalar registers the loop holds
  for (int b = (int)(lo + (hi - lo - 1) / 64 * 64); b >= (int)lo; b -= 64) {
    const int64_t i = (int64_t)b + lane;
    const bool live = i < hi;
    float a = 0.f, gw = 0.f, delta = 0.f, s = 0.f, nx = 0.f, ny = 0.f, nz = 0.f;
    if (live) {
      const float ts = t_starts[i], te = t_ends[i], w = weights[i];
      delta = te - ts;
      s = sdf[i];
      a = alphas[i];
      const int64_t at = i * C;
      gw = (g_weights ? g_weights[i] : 0.f) + go_opacity + go_depth * ((ts + te) * 0.5f);
#pragma unroll
      for (int c = 0; c < VOL_MAX_CHANNELS; c++) {
        if (c >= C) break;                                                 // C is uniform: a scalar branch, and go stays in registers
        gw += go[c] * values[at + c];
        if (g_values) g_values[at + c] = w * go[c];
      }
      if (normals) {
        nx = normals[3 * i];
        ny = normals[3 * i + 1];
        nz = normals[3 * i + 2];
      }
    }
    const float U = sdf_affine_scan(a, gw, live, lane, &carry);
    if (live) {
      const float g_alpha = trans[i] * (gw - U);
      const SdfAlpha f = sdf_alpha(s, delta, normals != nullptr, nx, ny, nz, dx, dy, dz, beta, rho);
      const float g_q = (f.q >= 0.f && f.q <= 1.f) ? g_alpha : 0.f;
      const float ce = f.c + SDF_EPS;
      const float g_xp = g_q * f.m / (ce * ce) * (f.c * (1.f - f.c));
      const float g_xn = -g_q / ce * (f.m * (1.f - f.m));
      g_sdf[i] = beta * (g_xp + g_xn);
      g_beta += g_xp * f.prev + g_xn * f.next;
      if (g_normals) {
        const float g_ic = beta * (g_xn - g_xp) * delta * 0.5f;
        const float slope = (-0.5f * f.t + 0.5f > 0.f ? 0.5f * (1.f - rho) : 0.f) + (f.t < 0.f ? rho : 0.f);
        const float g_t = g_ic * slope;
        g_normals[3 * i] = g_t * dx;
        g_normals[3 * i + 1] = g_t * dy;
        g_normals[3 * i + 2] = g_t * dz;
      }
    }
  }
  g_beta = vol_wave_sum(g_beta);
  if (lane == 0) g_inv_std_rays[r] = g_beta;
}

// ------------------------------------------------------------------------------------------------------------------------ host
static bool sdf_render_config(int64_t R, int64_t M, int32_t C, const float* values, float rho) {
  if (!vol_rows_ok(R, M) || C < 0 || C > VOL_MAX_CHANNELS || (values == nullptr) != (C == 0)) return false;
  if (M * (int64_t)(C > 1 ? C : 1) > (int64_t)INT32_MAX) return false;
  return isfinite(rho) && rho >= 0.f && rho <= 1.f;
}

extern "C" int gip_volume_alpha_weights_forward(const float* alphas, const int32_t* offsets, int64_t R, int64_t M, float* weights, float* trans,
                                                void* stream) {
  if (!vol_rows_ok(R, M)) return 1;
  if (R == 0 || M == 0) return 0;
  if (!alphas || !offsets || !weights || !trans) return 1;
  MESH_LAUNCH(volume_alpha_weights_forward_kernel, vol_ray_blocks(R), stream, alphas, offsets, R, M, weights, trans);
  return mesh_done();
}

extern "C" int gip_volume_alpha_weights_backward(const float* alphas, const float* trans, const float* g_weights, const int32_t* offsets,
                                                 int64_t R, int64_t M, float* g_alphas, void* stream) {
  if (!vol_rows_ok(R, M)) return 1;
  if (R == 0 || M == 0) return 0;
  if (!alphas || !trans || !g_weights || !offsets || !g_alphas) return 1;
  MESH_LAUNCH(volume_alpha_weights_backward_kernel, vol_ray_blocks(R), stream, alphas, trans, g_weights, offsets, R, M, g_alphas);
  return mesh_done();
}

extern "C" int gip_volume_sdf_render_forward(const float* sdf, const float* normals, const float* rays_d, const float* t_starts,
                                             const float* t_ends, const float* values, const int32_t* offsets, const float* inv_std,
                                             float cos_anneal_ratio, int64_t R, int64_t M, int32_t C, float* alphas, float* trans,
                                             float* weights, float* out, void* stream) {
  if (!sdf_render_config(R, M, C, values, cos_anneal_ratio)) return 1;
  if (R == 0 || M == 0) return 0;
  if (!sdf || !rays_d || !t_starts || !t_ends || !offsets || !inv_std || !alphas || !trans || !weights || !out) return 1;
  MESH_LAUNCH(volume_sdf_render_forward_kernel, vol_ray_blocks(R), stream, sdf, normals, rays_d, t_starts, t_ends, values, offsets, inv_std,
              cos_anneal_ratio, R, M, (int)C, alphas, trans, weights, out);
  return mesh_done();
}

extern "C" int gip_volume_sdf_render_backward(const float* sdf, const float* normals, const float* rays_d, const float* t_starts,
                                              const float* t_ends, const float* values, const int32_t* offsets, const float* inv_std,
                                              float cos_anneal_ratio, const float* alphas, const float* trans, const float* weights,
                                              const float* g_out, const float* g_weights, int64_t R, int64_t M, int32_t C, float* g_sdf,
                                              float* g_normals, float* g_values, float* g_inv_std_rays, void* stream) {
  if (!sdf_render_config(R, M, C, values, cos_anneal_ratio)) return 1;
  if (R == 0 || M == 0) return 0;
  if (!sdf || !rays_d || !t_starts || !t_ends || !offsets || !inv_std || !alphas || !trans || !weights || !g_out || !g_sdf ||
      !g_inv_std_rays || (g_normals && !normals))
    return 1;
  MESH_LAUNCH(volume_sdf_render_backward_kernel, vol_ray_blocks(R), stream, sdf, normals, rays_d, t_starts, t_ends, values, offsets, inv_std,
              cos_anneal_ratio, alphas, trans, weights, g_out, g_weights, R, M, (int)C, g_sdf, g_normals, g_values, g_inv_std_rays);
  return mesh_done();
}
