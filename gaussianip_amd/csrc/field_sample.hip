// field_sample.hip — the density field of field.hip asked for at arbitrary points: density, its gradient and the weight-blended
// colour of the Gaussians at a list of query points (mesh vertices: colours and smooth normals).  Linked into libgip_model.so.
//
// Definition (field.hip's, extended to other points): sources, normalisation xyz' = (xyz - center) * scale, the adjugate inverse A
// of Sigma with 1 / (det + 1e-24), block membership (centre STRICTLY inside the block's box relaxed by `margin`) are exactly those
// of gip_density_field.  A query point x (normalised coordinates) comes with the block b it is evaluated in — the caller decides
// the block and hands the points over grouped by block (block_start: exclusive offsets).  With d = x - mu', power = -0.5 d^T A d,
// w = opacity * exp(power) (a positive power counting as weight 0), summed over the members of b:
//     density = sum w        gradient = sum w * (-A d)   (d density / d x, normalised space)        color_sum = sum w * rgb
// The raw sums are written; color_sum / density is the caller's business.
//
//   sample_prepare_kernel  this file's copy of field_prepare_kernel (a kernel cannot be launched across translation units without
//                          relocatable device code): the same 10-float record and the same six-field block-range word, in the
//                          same operand order, so membership is identical.
//   sample_eval_kernel     one workgroup per block.  A block WITHOUT query points returns before it reads a range word (surface
//                          vertices occupy a thin shell of blocks).  Otherwise PPT points per lane stay in registers (point k * 256 +
//                          tid of the pass in slot k; slots past the pass's count are skipped by a workgroup-uniform branch), with a
//                          further pass when the block holds more than 256 * PPT points.  Members are found as in field_eval_kernel:
//                          the range words are walked 1024 per trip and compacted IN INDEX ORDER (ballot + popcount) into an LDS
//                          list, the listed records staged in LDS 256 at a time; each batch is summed on its own and then added
//                          to the point's totals.  List capacity, trip and batch sizes are field.hip's, and `power` is the same
//                          explicit fmaf chain, so at a grid point the density is bit for bit the voxel of gip_density_field.
//                          The per-point order is the Gaussians' order in memory: no float atomic, two runs are bitwise equal.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gip_model.h"

#define SAMPLE_THREADS 256
#define SAMPLE_WAVES (SAMPLE_THREADS / 64)
#define SAMPLE_SUB 4                                  // range words tested per thread per trip
#define SAMPLE_CHUNK (SAMPLE_THREADS * SAMPLE_SUB)    // 1024
#define SAMPLE_CAP 2048                               // capacity of the LDS member list; flushed when a trip might overflow it
#define SAMPLE_BATCH 256                              // records staged in LDS at a time
#define SAMPLE_REC 10                                 // floats of a record: xyz' (3), inverse covariance (6), opacity
#define SAMPLE_MAX_BLOCKS 1024                        // per axis: the range word has 10 bits per field
#define SAMPLE_PPT 4                                  // points per lane and pass: 7 sums + 7 batch sums + 3 coordinates each

// ------------------------------------------------------------------------------------------------------------------ prepare
__global__ void __launch_bounds__(SAMPLE_THREADS)
sample_prepare_kernel(const float* __restrict__ xyz, const float* __restrict__ opacity, const float* __restrict__ scaling,
                      const float* __restrict__ rotation, int64_t P, const float* __restrict__ center, float scale,
                      const float* __restrict__ grid, int R, int nb, float margin, float* __restrict__ rec, uint64_t* __restrict__ range) {
  const int64_t g = (int64_t)blockIdx.x * SAMPLE_THREADS + threadIdx.x;
  if (g >= P) return;
  const int s = R / nb;
  float p[3], sd[3];
#pragma unroll
  for (int a = 0; a < 3; a++) {
    p[a] = (xyz[g * 3 + a] - center[a]) * scale;
    sd[a] = scaling[g * 3 + a] * scale;
  }
  // build_rotation: the raw quaternion divided by its norm
  const float q0 = rotation[g * 4], q1 = rotation[g * 4 + 1], q2 = rotation[g * 4 + 2], q3 = rotation[g * 4 + 3];
  const float norm = sqrtf(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
  const float r = q0 / norm, x = q1 / norm, y = q2 / norm, z = q3 / norm;
  float Rm[3][3];
  Rm[0][0] = 1.f - 2.f * (y * y + z * z);
  Rm[0][1] = 2.f * (x * y - r * z);
  Rm[0][2] = 2.f * (x * z + r * y);
  Rm[1][0] = 2.f * (x * y + r * z);
  Rm[1][1] = 1.f - 2.f * (x * x + z * z);
  Rm[1][2] = 2.f * (y * z - r * x);
  Rm[2][0] = 2.f * (x * z - r * y);
  Rm[2][1] = 2.f * (y * z + r * x);
  Rm[2][2] = 1.f - 2.f * (x * x + y * y);
  float L[3][3];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) L[i][j] = Rm[i][j] * sd[j];
  float S[3][3];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = i; j < 3; j++) S[i][j] = L[i][0] * L[j][0] + L[i][1] * L[j][1] + L[i][2] * L[j][2];
  const float a = S[0][0], b = S[0][1], c = S[0][2], d = S[1][1], e = S[1][2], f = S[2][2];
  const float inv_det = 1.f / (a * d * f + 2.f * e * c * b - e * e * a - c * c * d - b * b * f + 1e-24f);
  float* o = rec + g * SAMPLE_REC;
  o[0] = p[0];
  o[1] = p[1];
  o[2] = p[2];
  o[3] = (d * f - e * e) * inv_det;   // inv_a
  o[4] = (e * c - b * f) * inv_det;   // inv_b
  o[5] = (e * b - c * d) * inv_det;   // inv_c
  o[6] = (a * f - c * c) * inv_det;   // inv_d
  o[7] = (b * c - e * a) * inv_det;   // inv_e
  o[8] = (a * d - b * b) * inv_det;   // inv_f
  o[9] = opacity[g];
  // the blocks this centre belongs to, per axis: vmin = first - margin < x' < last + margin = vmax, in float32 like the reference
  uint64_t word = 0;
#pragma unroll
  for (int ax = 0; ax < 3; ax++) {
    int first = 1, last = 0;
    bool any = false;
    for (int bk = 0; bk < nb; bk++) {
      const float vmin = grid[bk * s] - margin, vmax = grid[bk * s + s - 1] + margin;
      if (p[ax] < vmax && p[ax] > vmin) {
        if (!any) first = bk;
        last = bk;
        any = true;
      }
    }
    word |= ((uint64_t)first | ((uint64_t)last << 10)) << (20 * ax);
  }
  range[g] = word;
}

// ------------------------------------------------------------------------------------------------------------------ evaluate
template <int PPT, bool COLOR>
__global__ void __launch_bounds__(SAMPLE_THREADS)
sample_eval_kernel(const float* __restrict__ rec, const uint64_t* __restrict__ range, const float* __restrict__ rgb, int64_t P, int nb,
                   const float* __restrict__ points, const int32_t* __restrict__ block_start, int V, float* __restrict__ density,
                   float* __restrict__ gradient, float* __restrict__ color_sum) {
  // the block's points; clipped to [0, V] so that no offset, whatever the caller wrote there, leads outside the arrays
  const int first = max(block_start[blockIdx.x], 0), end = min(block_start[blockIdx.x + 1], V);
  if (end <= first) return;   // no query point here: not a single range word is read
  __shared__ int s_idx[SAMPLE_CAP];
  __shared__ float4 s_rec[SAMPLE_BATCH][COLOR ? 4 : 3];
  __shared__ int s_cnt[2][SAMPLE_SUB][SAMPLE_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bz = blockIdx.x % nb, by = (blockIdx.x / nb) % nb, bx = blockIdx.x / (nb * nb);
  const uint64_t lt = lane ? (~0ull >> (64 - lane)) : 0ull;   // lanes below this one

  for (int p0 = first; p0 < end; p0 += SAMPLE_THREADS * PPT) {      // one pass unless the block holds more than 256 * PPT points
    const int slots = (min(end - p0, SAMPLE_THREADS * PPT) + SAMPLE_THREADS - 1) / SAMPLE_THREADS;   // slots in use: workgroup-uniform
    float px[PPT], py[PPT], pz[PPT], acc[PPT][COLOR ? 7 : 4];
    int at[PPT];
#pragma unroll
    for (int k = 0; k < PPT; k++) {
      const int v = p0 + k * SAMPLE_THREADS + tid;
      const int vc = v < end ? v : first;
      px[k] = points[(int64_t)vc * 3];
      py[k] = points[(int64_t)vc * 3 + 1];
      pz[k] = points[(int64_t)vc * 3 + 2];
      at[k] = v < end ? v : -1;
#pragma unroll
      for (int c = 0; c < (COLOR ? 7 : 4); c++) acc[k][c] = 0.f;
    }
    int staged = 0, par = 0;
    for (int64_t base = 0; base < P; base += SAMPLE_CHUNK) {
      // ---- which of the next 1024 Gaussians belong to this block; their indices appended to s_idx in index order
      uint64_t bal[SAMPLE_SUB];
      bool mine[SAMPLE_SUB];
#pragma unroll
      for (int i = 0; i < SAMPLE_SUB; i++) {
        const int64_t g = base + i * SAMPLE_THREADS + tid;
        bool m = false;
        if (g < P) {
          const uint64_t w = range[g];
          const int x0 = (int)(w & 1023), x1 = (int)((w >> 10) & 1023), y0 = (int)((w >> 20) & 1023), y1 = (int)((w >> 30) & 1023),
                    z0 = (int)((w >> 40) & 1023), z1 = (int)((w >> 50) & 1023);
          m = bx >= x0 && bx <= x1 && by >= y0 && by <= y1 && bz >= z0 && bz <= z1;
        }
        mine[i] = m;
        bal[i] = __ballot(m);
        if (lane == 0) s_cnt[par][i][wave] = __popcll(bal[i]);
      }
      __syncthreads();
      int run = staged;
#pragma unroll
      for (int i = 0; i < SAMPLE_SUB; i++) {
        int off = 0;
#pragma unroll
        for (int w = 0; w < SAMPLE_WAVES; w++) {
          if (w == wave) off = run;
          run += s_cnt[par][i][w];
        }
        if (mine[i]) s_idx[off + __popcll(bal[i] & lt)] = (int)(base + i * SAMPLE_THREADS + tid);
      }
      staged = run;   // the same value in every thread; <= SAMPLE_CAP because a flush leaves at most SAMPLE_CAP - SAMPLE_CHUNK behind
      par ^= 1;
      if (staged <= SAMPLE_CAP - SAMPLE_CHUNK && base + SAMPLE_CHUNK < P) continue;
      // ---- flush: add the listed Gaussians to this lane's points, 256 records at a time
      for (int sb = 0; sb < staged; sb += SAMPLE_BATCH) {
        __syncthreads();   // s_idx is complete; the previous batch's records are no longer read
        const int n = min(SAMPLE_BATCH, staged - sb);
        if (tid < n) {
          const int64_t gi = s_idx[sb + tid];
          const float* r = rec + gi * SAMPLE_REC;
          // power = dx (A dx + B dy + C dz) + dy (D dy + E dz) + dz (F dz): the scalings by -0.5 and -1 are exact
          s_rec[tid][0] = make_float4(r[0], r[1], r[2], r[9]);
          s_rec[tid][1] = make_float4(-0.5f * r[3], -r[4], -r[5], -0.5f * r[6]);
          s_rec[tid][2] = make_float4(-r[7], -0.5f * r[8], 0.f, 0.f);
          if (COLOR) s_rec[tid][3] = make_float4(rgb[gi * 3], rgb[gi * 3 + 1], rgb[gi * 3 + 2], 0.f);
        }
        __syncthreads();
        float part[PPT][COLOR ? 7 : 4];
#pragma unroll
        for (int k = 0; k < PPT; k++)
#pragma unroll
          for (int c = 0; c < (COLOR ? 7 : 4); c++) part[k][c] = 0.f;
        for (int j = 0; j < n; j++) {
          const float4 c0 = s_rec[j][0], c1 = s_rec[j][1], c2 = s_rec[j][2];
          float4 c3 = make_float4(0.f, 0.f, 0.f, 0.f);
          if (COLOR) c3 = s_rec[j][3];
#pragma unroll
          for (int k = 0; k < PPT; k++) {
            if (k >= slots) continue;
            const float dx = px[k] - c0.x, dy = py[k] - c0.y, dz = pz[k] - c0.z;
            const float t0 = fmaf(c1.z, dz, fmaf(c1.y, dy, c1.x * dx));   // -(A/2 dx + B dy + C dz)
            const float t1 = fmaf(c2.x, dz, c1.w * dy);                   // -(D/2 dy + E dz)
            const float t2 = c2.y * dz;                                   // -(F/2 dz)
            const float power = fmaf(dx, t0, fmaf(dy, t1, dz * t2));
#ifdef FIELD_PRECISE_EXP
            const float e = power > 0.f ? 0.f : expf(power);
#else
            const float e = power > 0.f ? 0.f : __expf(power);
#endif
            part[k][0] = fmaf(c0.w, e, part[k][0]);
            // -A d = (-(A dx + B dy + C dz), -(B dx + D dy + E dz), -(C dx + E dy + F dz)) from the halves above
            const float w = c0.w * e;
            part[k][1] = fmaf(w, fmaf(c1.x, dx, t0), part[k][1]);
            part[k][2] = fmaf(w, fmaf(c1.y, dx, fmaf(c1.w, dy, t1)), part[k][2]);
            part[k][3] = fmaf(w, fmaf(c1.z, dx, fmaf(c2.x, dy, t2 + t2)), part[k][3]);
            if (COLOR) {
              part[k][4] = fmaf(w, c3.x, part[k][4]);
              part[k][5] = fmaf(w, c3.y, part[k][5]);
              part[k][6] = fmaf(w, c3.z, part[k][6]);
            }
          }
        }
#pragma unroll
        for (int k = 0; k < PPT; k++)
#pragma unroll
          for (int c = 0; c < (COLOR ? 7 : 4); c++) acc[k][c] += part[k][c];
      }
      staged = 0;
    }
#pragma unroll
    for (int k = 0; k < PPT; k++) {
      if (at[k] < 0) continue;
      const int64_t o = at[k];
      density[o] = acc[k][0];
      if (gradient) {
        gradient[o * 3] = acc[k][1];
        gradient[o * 3 + 1] = acc[k][2];
        gradient[o * 3 + 2] = acc[k][3];
      }
      if (COLOR) {
        color_sum[o * 3] = acc[k][4];
        color_sum[o * 3 + 1] = acc[k][5];
        color_sum[o * 3 + 2] = acc[k][6];
      }
    }
    __syncthreads();   // a further pass reuses s_idx and s_cnt
  }
}

// the limits of gip_density_field (field.hip: field_shape_ok)
static int sample_shape_ok(int64_t P, int32_t R, int32_t nb) {
  if (P < 0 || P > INT32_MAX || R < 1 || nb < 1 || nb > SAMPLE_MAX_BLOCKS || R % nb != 0) return 0;
  if ((int64_t)nb * nb * nb > INT32_MAX) return 0;
  return 1;
}

extern "C" int gip_field_sample_workspace_size(int64_t P, int32_t R, int32_t num_blocks, size_t* bytes) {
  if (!bytes || !sample_shape_ok(P, R, num_blocks)) return 1;
  // records [P, 10] float, then range words [P] (8-byte aligned: 40 P is a multiple of 8)
  *bytes = (size_t)P * (SAMPLE_REC * sizeof(float) + sizeof(uint64_t));
  return 0;
}

extern "C" int gip_field_sample(const float* xyz, const float* opacity, const float* scaling, const float* rotation, const float* rgb,
                                int64_t P, const float* center, float scale, const float* grid, int32_t R, int32_t num_blocks,
                                float margin, const float* points, const int32_t* block_start, int64_t V, void* workspace,
                                size_t workspace_bytes, float* density, float* gradient, float* color_sum, void* stream) {
  size_t need = 0;
  if (gip_field_sample_workspace_size(P, R, num_blocks, &need) != 0 || V < 0 || V > INT32_MAX) return 1;
  if (color_sum && !rgb) return 1;
  if (V == 0) return 0;
  if (!points || !block_start || !density) return 1;
  hipStream_t st = (hipStream_t)stream;
  if (P == 0) {   // no sources: every sum is empty
    hipError_t err = hipMemsetAsync(density, 0, (size_t)V * sizeof(float), st);
    if (err == hipSuccess && gradient) err = hipMemsetAsync(gradient, 0, (size_t)V * 3 * sizeof(float), st);
    if (err == hipSuccess && color_sum) err = hipMemsetAsync(color_sum, 0, (size_t)V * 3 * sizeof(float), st);
    return err == hipSuccess ? 0 : 3;
  }
  if (!xyz || !opacity || !scaling || !rotation || !center || !grid || !workspace || workspace_bytes < need) return 1;
  float* rec = (float*)workspace;
  uint64_t* range = (uint64_t*)(rec + (size_t)P * SAMPLE_REC);
  hipLaunchKernelGGL(sample_prepare_kernel, dim3((unsigned)((P + SAMPLE_THREADS - 1) / SAMPLE_THREADS)), dim3(SAMPLE_THREADS), 0, st, xyz,
                     opacity, scaling, rotation, P, center, scale, grid, (int)R, (int)num_blocks, margin, rec, range);
  const dim3 blocks((unsigned)(num_blocks * num_blocks * num_blocks));
  if (color_sum)
    hipLaunchKernelGGL((sample_eval_kernel<SAMPLE_PPT, true>), blocks, dim3(SAMPLE_THREADS), 0, st, rec, range, rgb, P, (int)num_blocks,
                       points, block_start, (int)V, density, gradient, color_sum);
  else
    hipLaunchKernelGGL((sample_eval_kernel<SAMPLE_PPT, false>), blocks, dim3(SAMPLE_THREADS), 0, st, rec, range, rgb, P, (int)num_blocks,
                       points, block_start, (int)V, density, gradient, color_sum);
  return hipGetLastError() == hipSuccess ? 0 : 3;
}
