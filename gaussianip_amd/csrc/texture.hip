// texture.hip — the colour of the Gaussians baked into a UV texture of a triangle mesh: the pair evaluation of field_sample.hip at
// the texels of an atlas in which every face owns a right-isosceles triangle of texels (gaussianip_amd/utils/texture.py states the
// layout; DESIGN.md "Baking a texture").  Linked into libgip_model.so.
//
// Definition: sources, normalisation, inverse covariance, blocks, membership and `margin` are gip_density_field's.  Face f lives in
// cell q = f / 2 (row q / n, column q % n, n = T / cell cells per row) as half h = f & 1; a texel with cell-local indices (i, j)
// belongs to half (i + j >= cell).  With local indices (li, lj) = (i, j) for half 0 and (cell - 1 - i, cell - 1 - j) for half 1 and the
// leg b = cell - 3, the texel's point is p = v0 + (li / b) (v1 - v0) + (lj / b) (v2 - v0) on the normalised vertices, in float32 in
// that operand order (texels past the hypotenuse: the plane extrapolated).  Every texel of a face is evaluated in the face's block,
// which the caller decides (face_order: face ids grouped by block; block_start: offsets into it):
//     density = sum w        color_sum = sum w * rgb        w = opacity * exp(power), a positive power counting as 0
// The raw sums are written; unowned texels are not touched.
//
//   texture_prepare_kernel  this file's copy of field_prepare_kernel (a kernel cannot be launched across translation units without
//                           relocatable device code): the same record and block-range word, so membership is identical.
//   texture_eval_kernel     grid = block x slice.  A block's texel slots ((faces of the block) * cell (cell + 1) / 2; slot -> (li, lj)
//                           by folding the triangle's rows r and cell - r [cell odd] or cell - 1 - r [cell even] into one row of a
//                           rectangle; the odd face skips the cell slots of the diagonal li + lj = cell - 1, which half 0 owns) are cut
//                           into passes of 256 * PPT; slice s takes passes s, s + slices, ...  A workgroup whose first pass lies
//                           past the block's count returns before it reads a range word.  A lane derives its texels' faces, local
//                           indices and points in registers: no point array is read, and the sums go straight into the texture.
//                           The walk over the Gaussians is sample_eval_kernel's, statement for statement (trips of 1024 range
//                           words, in-order compaction into a list of 2048, batches of 256, each batch summed on its own, the same
//                           explicit fmaf chain): given the same points and blocks the sums are gip_field_sample's bit for bit,
//                           whatever `slices` is.  Only density and colour are accumulated: 3 + 4 + 4 registers per point.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gip_model.h"

#define TEX_THREADS 256
#define TEX_WAVES (TEX_THREADS / 64)
#define TEX_SUB 4                               // range words tested per thread per trip
#define TEX_CHUNK (TEX_THREADS * TEX_SUB)       // 1024
#define TEX_CAP 2048                            // capacity of the LDS member list; flushed when a trip might overflow it
#define TEX_BATCH 256                           // records staged in LDS at a time
#define TEX_REC 10                              // floats of a record: xyz' (3), inverse covariance (6), opacity
#define TEX_MAX_BLOCKS 1024                     // per axis: the range word has 10 bits per field
#define TEX_PPT 4                               // texels per lane and pass: 4 sums + 4 batch sums + 3 coordinates each
#define TEX_PASS (TEX_THREADS * TEX_PPT)        // texel slots of one pass
#define TEX_MAX_SIZE 16384
#define TEX_MAX_SLICES 65535                    // the grid's second dimension
#define TEX_AUTO_SLICES 1024

// ------------------------------------------------------------------------------------------------------------------ prepare
__global__ void __launch_bounds__(TEX_THREADS)
texture_prepare_kernel(const float* __restrict__ xyz, const float* __restrict__ opacity, const float* __restrict__ scaling,
                       const float* __restrict__ rotation, int64_t P, const float* __restrict__ center, float scale,
                       const float* __restrict__ grid, int R, int nb, float margin, float* __restrict__ rec, uint64_t* __restrict__ range) {
  const int64_t g = (int64_t)blockIdx.x * TEX_THREADS + threadIdx.x;
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
  float* o = rec + g * TEX_REC;
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
template <int PPT>
__global__ void __launch_bounds__(TEX_THREADS)
texture_eval_kernel(const float* __restrict__ rec, const uint64_t* __restrict__ range, const float* __restrict__ rgb, int64_t P, int nb,
                    const float* __restrict__ vertices, int V, const int32_t* __restrict__ faces, int F,
                    const int32_t* __restrict__ face_order, const int32_t* __restrict__ block_start, int T, int cell,
                    float* __restrict__ density, float* __restrict__ color_sum) {
  // the block's faces; clipped to [0, F] so that no offset, whatever the caller wrote there, leads outside the arrays
  const int first = max(block_start[blockIdx.x], 0), end = min(block_start[blockIdx.x + 1], F);
  if (end <= first) return;   // no face here: not a single range word is read
  const int per_face = cell * (cell + 1) / 2;
  const int total = (end - first) * per_face;   // < 2^31: F * per_face <= (T / cell)^2 * cell * (cell + 1) <= 1.25 T^2
  if ((int64_t)blockIdx.y * (TEX_THREADS * PPT) >= total) return;   // this slice has no pass: nothing read either
  __shared__ int s_idx[TEX_CAP];
  __shared__ float4 s_rec[TEX_BATCH][4];
  __shared__ int s_cnt[2][TEX_SUB][TEX_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bz = blockIdx.x % nb, by = (blockIdx.x / nb) % nb, bx = blockIdx.x / (nb * nb);
  const uint64_t lt = lane ? (~0ull >> (64 - lane)) : 0ull;   // lanes below this one
  const int n = T / cell, leg = cell - 3, fold = cell | 1;    // fold: the width of the rectangle the triangle's rows are folded into
  const float fleg = (float)leg;

  for (int p0 = (int)blockIdx.y * (TEX_THREADS * PPT); p0 < total; p0 += (int)gridDim.y * (TEX_THREADS * PPT)) {
    const int slots = (min(total - p0, TEX_THREADS * PPT) + TEX_THREADS - 1) / TEX_THREADS;   // slots in use: workgroup-uniform
    float px[PPT], py[PPT], pz[PPT], acc[PPT][4];
    int at[PPT];
#pragma unroll
    for (int k = 0; k < PPT; k++) {
      const int t = p0 + k * TEX_THREADS + tid;
      const int tc = t < total ? t : p0;
      const int fi = tc / per_face, slot = tc - fi * per_face;
      const int f = min(max(face_order[first + fi], 0), F - 1);
      const int h = f & 1, q = f >> 1;
      // slot -> (li, lj), li + lj <= cell - 1
      const int r = slot / fold, kk = slot - r * fold;
      const bool head = kk < cell - r;
      const int lj = head ? r : ((cell & 1) ? cell - r : cell - 1 - r);
      const int li = head ? kk : kk - (cell - r);
      const int row = q / n, col = q - row * n;
      const int x = col * cell + (h ? cell - 1 - li : li), y = row * cell + (h ? cell - 1 - lj : lj);
      const bool owned = t < total && !(h && li + lj == cell - 1);
      at[k] = owned ? y * T + x : -1;
      const int i0 = min(max(faces[(int64_t)f * 3], 0), V - 1), i1 = min(max(faces[(int64_t)f * 3 + 1], 0), V - 1),
                i2 = min(max(faces[(int64_t)f * 3 + 2], 0), V - 1);
      const float a = (float)li / fleg, b = (float)lj / fleg;
      const float* v0 = vertices + (int64_t)i0 * 3;
      const float* v1 = vertices + (int64_t)i1 * 3;
      const float* v2 = vertices + (int64_t)i2 * 3;
      px[k] = v0[0] + a * (v1[0] - v0[0]) + b * (v2[0] - v0[0]);
      py[k] = v0[1] + a * (v1[1] - v0[1]) + b * (v2[1] - v0[1]);
      pz[k] = v0[2] + a * (v1[2] - v0[2]) + b * (v2[2] - v0[2]);
#pragma unroll
      for (int c = 0; c < 4; c++) acc[k][c] = 0.f;
    }
    int staged = 0, par = 0;
    for (int64_t base = 0; base < P; base += TEX_CHUNK) {
      // ---- which of the next 1024 Gaussians belong to this block; their indices appended to s_idx in index order
      uint64_t bal[TEX_SUB];
      bool mine[TEX_SUB];
#pragma unroll
      for (int i = 0; i < TEX_SUB; i++) {
        const int64_t g = base + i * TEX_THREADS + tid;
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
      for (int i = 0; i < TEX_SUB; i++) {
        int off = 0;
#pragma unroll
        for (int w = 0; w < TEX_WAVES; w++) {
          if (w == wave) off = run;
          run += s_cnt[par][i][w];
        }
        if (mine[i]) s_idx[off + __popcll(bal[i] & lt)] = (int)(base + i * TEX_THREADS + tid);
      }
      staged = run;   // the same value in every thread; <= TEX_CAP because a flush leaves at most TEX_CAP - TEX_CHUNK behind
      par ^= 1;
      if (staged <= TEX_CAP - TEX_CHUNK && base + TEX_CHUNK < P) continue;
      // ---- flush: add the listed Gaussians to this lane's texels, 256 records at a time
      for (int sb = 0; sb < staged; sb += TEX_BATCH) {
        __syncthreads();   // s_idx is complete; the previous batch's records are no longer read
        const int nrec = min(TEX_BATCH, staged - sb);
        if (tid < nrec) {
          const int64_t gi = s_idx[sb + tid];
          const float* r = rec + gi * TEX_REC;
          // power = dx (A dx + B dy + C dz) + dy (D dy + E dz) + dz (F dz): the scalings by -0.5 and -1 are exact
          s_rec[tid][0] = make_float4(r[0], r[1], r[2], r[9]);
          s_rec[tid][1] = make_float4(-0.5f * r[3], -r[4], -r[5], -0.5f * r[6]);
          s_rec[tid][2] = make_float4(-r[7], -0.5f * r[8], 0.f, 0.f);
          s_rec[tid][3] = make_float4(rgb[gi * 3], rgb[gi * 3 + 1], rgb[gi * 3 + 2], 0.f);
        }
        __syncthreads();
        float part[PPT][4];
#pragma unroll
        for (int k = 0; k < PPT; k++)
#pragma unroll
          for (int c = 0; c < 4; c++) part[k][c] = 0.f;
        for (int j = 0; j < nrec; j++) {
          const float4 c0 = s_rec[j][0], c1 = s_rec[j][1], c2 = s_rec[j][2], c3 = s_rec[j][3];
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
            const float w = c0.w * e;
            part[k][1] = fmaf(w, c3.x, part[k][1]);
            part[k][2] = fmaf(w, c3.y, part[k][2]);
            part[k][3] = fmaf(w, c3.z, part[k][3]);
          }
        }
#pragma unroll
        for (int k = 0; k < PPT; k++)
#pragma unroll
          for (int c = 0; c < 4; c++) acc[k][c] += part[k][c];
      }
      staged = 0;
    }
#pragma unroll
    for (int k = 0; k < PPT; k++) {
      if (at[k] < 0) continue;
      const int64_t o = at[k];
      density[o] = acc[k][0];
      color_sum[o * 3] = acc[k][1];
      color_sum[o * 3 + 1] = acc[k][2];
      color_sum[o * 3 + 2] = acc[k][3];
    }
    __syncthreads();   // a further pass reuses s_idx and s_cnt
  }
}

// the limits of gip_density_field (field.hip: field_shape_ok)
static int texture_shape_ok(int64_t P, int32_t R, int32_t nb) {
  if (P < 0 || P > INT32_MAX || R < 1 || nb < 1 || nb > TEX_MAX_BLOCKS || R % nb != 0) return 0;
  if ((int64_t)nb * nb * nb > INT32_MAX) return 0;
  return 1;
}

extern "C" int gip_texture_bake_workspace_size(int64_t P, int32_t R, int32_t num_blocks, size_t* bytes) {
  if (!bytes || !texture_shape_ok(P, R, num_blocks)) return 1;
  // records [P, 10] float, then range words [P] (8-byte aligned: 40 P is a multiple of 8)
  *bytes = (size_t)P * (TEX_REC * sizeof(float) + sizeof(uint64_t));
  return 0;
}

extern "C" int gip_texture_bake(const float* xyz, const float* opacity, const float* scaling, const float* rotation, const float* rgb,
                                int64_t P, const float* center, float scale, const float* grid, int32_t R, int32_t num_blocks,
                                float margin, const float* vertices, int64_t V, const int32_t* faces, int64_t F,
                                const int32_t* face_order, const int32_t* block_start, int32_t T, int32_t cell, int32_t slices,
                                void* workspace, size_t workspace_bytes, float* density, float* color_sum, void* stream) {
  size_t need = 0;
  if (gip_texture_bake_workspace_size(P, R, num_blocks, &need) != 0) return 1;
  if (F < 0 || F > INT32_MAX || V < 0 || V > INT32_MAX) return 1;
  if (T < 4 || T > TEX_MAX_SIZE || cell < 4 || cell > T) return 1;
  const int64_t n = T / cell;
  if (2 * n * n < F) return 1;
  if (slices < 0 || slices > TEX_MAX_SLICES) return 1;
  if (F == 0) return 0;
  if (!vertices || V == 0 || !faces || !face_order || !block_start || !density || !color_sum) return 1;
  hipStream_t st = (hipStream_t)stream;
  if (P == 0) {   // no sources: every sum is empty
    hipError_t err = hipMemsetAsync(density, 0, (size_t)T * T * sizeof(float), st);
    if (err == hipSuccess) err = hipMemsetAsync(color_sum, 0, (size_t)T * T * 3 * sizeof(float), st);
    return err == hipSuccess ? 0 : 3;
  }
  if (!xyz || !opacity || !scaling || !rotation || !rgb || !center || !grid || !workspace || workspace_bytes < need) return 1;
  if (slices == 0) {   // without a read of the blocks' counts: what one block holding every face would need
    const int64_t passes = (F * (cell * (cell + 1) / 2) + TEX_PASS - 1) / TEX_PASS;
    slices = (int32_t)(passes < TEX_AUTO_SLICES ? passes : TEX_AUTO_SLICES);
  }
  float* rec = (float*)workspace;
  uint64_t* range = (uint64_t*)(rec + (size_t)P * TEX_REC);
  hipLaunchKernelGGL(texture_prepare_kernel, dim3((unsigned)((P + TEX_THREADS - 1) / TEX_THREADS)), dim3(TEX_THREADS), 0, st, xyz, opacity,
                     scaling, rotation, P, center, scale, grid, (int)R, (int)num_blocks, margin, rec, range);
  const dim3 blocks((unsigned)(num_blocks * num_blocks * num_blocks), (unsigned)slices);
  hipLaunchKernelGGL((texture_eval_kernel<TEX_PPT>), blocks, dim3(TEX_THREADS), 0, st, rec, range, rgb, P, (int)num_blocks, vertices, (int)V,
                     faces, (int)F, face_order, block_start, (int)T, (int)cell, density, color_sum);
  return hipGetLastError() == hipSuccess ? 0 : 3;
}
