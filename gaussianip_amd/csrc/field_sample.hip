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
// The Gaussians are prepared by field.hip's kernel (field_prepare_launch): the same records and range words, so membership is
// gip_density_field's.
//   sample_eval_kernel     one workgroup per block.  A block WITHOUT query points returns before it reads a range word (surface
//                          vertices occupy a thin shell of blocks).  Otherwise PPT points per lane stay in registers (point k * 256 +
//                          tid of the pass in slot k; slots past the pass's count are skipped by a workgroup-uniform branch), with a
//                          further pass when the block holds more than 256 * PPT points.  Members are found and pairs evaluated by
//                          the walk that field_eval_kernel uses (field_common.h: field_walk), so at a grid point the density is bit
//                          for bit the voxel of gip_density_field; this kernel's own part is the block's point range and seven
//                          (without colour: four) sums per pair.  The per-point order is the Gaussians' order in memory: no float
//                          atomic, two runs are bitwise equal.
#include "field_common.h"

#define SAMPLE_PPT 4                                  // points per lane and pass: 7 sums + 7 batch sums + 3 coordinates each

template <int PPT, bool COLOR>
__global__ void __launch_bounds__(FIELD_THREADS)
sample_eval_kernel(const float* __restrict__ rec, const uint64_t* __restrict__ range, const float* __restrict__ rgb, int64_t P, int nb,
                   const float* __restrict__ points, const int32_t* __restrict__ block_start, int V, float* __restrict__ density,
                   float* __restrict__ gradient, float* __restrict__ color_sum) {
  // the block's points; clipped to [0, V] so that no offset, whatever the caller wrote there, leads outside the arrays
  const int first = max(block_start[blockIdx.x], 0), end = min(block_start[blockIdx.x + 1], V);
  if (end <= first) return;   // no query point here: not a single range word is read
  __shared__ FieldLds<COLOR> lds;
  constexpr int SUMS = COLOR ? 7 : 4;
  const int tid = threadIdx.x;
  const int bz = blockIdx.x % nb, by = (blockIdx.x / nb) % nb, bx = blockIdx.x / (nb * nb);

  for (int p0 = first; p0 < end; p0 += FIELD_THREADS * PPT) {      // one pass unless the block holds more than 256 * PPT points
    const int slots = (min(end - p0, FIELD_THREADS * PPT) + FIELD_THREADS - 1) / FIELD_THREADS;   // slots in use: workgroup-uniform
    float px[PPT], py[PPT], pz[PPT], acc[PPT][SUMS];
    int at[PPT];
#pragma unroll
    for (int k = 0; k < PPT; k++) {
      const int v = p0 + k * FIELD_THREADS + tid;
      const int vc = v < end ? v : first;
      px[k] = points[(int64_t)vc * 3];
      py[k] = points[(int64_t)vc * 3 + 1];
      pz[k] = points[(int64_t)vc * 3 + 2];
      at[k] = v < end ? v : -1;
#pragma unroll
      for (int c = 0; c < SUMS; c++) acc[k][c] = 0.f;
    }
    field_walk<PPT, SUMS, COLOR>(lds, rec, range, rgb, P, bx, by, bz, px, py, pz, slots, acc, [](const FieldPair& q, float (&part)[SUMS]) {
      part[0] = fmaf(q.c0.w, q.e, part[0]);
      // -A d = (-(A dx + B dy + C dz), -(B dx + D dy + E dz), -(C dx + E dy + F dz)) from the halves t0, t1, t2
      const float w = q.c0.w * q.e;
      part[1] = fmaf(w, fmaf(q.c1.x, q.dx, q.t0), part[1]);
      part[2] = fmaf(w, fmaf(q.c1.y, q.dx, fmaf(q.c1.w, q.dy, q.t1)), part[2]);
      part[3] = fmaf(w, fmaf(q.c1.z, q.dx, fmaf(q.c2.x, q.dy, q.t2 + q.t2)), part[3]);
      if constexpr (COLOR) {
        part[4] = fmaf(w, q.c3.x, part[4]);
        part[5] = fmaf(w, q.c3.y, part[5]);
        part[6] = fmaf(w, q.c3.z, part[6]);
      }
    });
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
      if constexpr (COLOR) {
        color_sum[o * 3] = acc[k][4];
        color_sum[o * 3 + 1] = acc[k][5];
        color_sum[o * 3 + 2] = acc[k][6];
      }
    }
  }
}

extern "C" int gip_field_sample_workspace_size(int64_t P, int32_t R, int32_t num_blocks, size_t* bytes) {
  return field_workspace_size(P, R, num_blocks, bytes);
}

extern "C" int gip_field_sample(const float* xyz, const float* opacity, const float* scaling, const float* rotation, const float* rgb,
                                int64_t P, const float* center, float scale, const float* grid, int32_t R, int32_t num_blocks,
                                float margin, const float* points, const int32_t* block_start, int64_t V, void* workspace,
                                size_t workspace_bytes, float* density, float* gradient, float* color_sum, void* stream) {
  size_t need = 0;
  if (field_workspace_size(P, R, num_blocks, &need) != 0 || V < 0 || V > INT32_MAX) return 1;
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
  const FieldPrepared prep = field_workspace_split(workspace, P);
  field_prepare_launch(xyz, opacity, scaling, rotation, P, center, scale, grid, (int)R, (int)num_blocks, margin, prep, st);
  const dim3 blocks((unsigned)(num_blocks * num_blocks * num_blocks));
  if (color_sum)
    hipLaunchKernelGGL((sample_eval_kernel<SAMPLE_PPT, true>), blocks, dim3(FIELD_THREADS), 0, st, prep.rec, prep.range, rgb, P,
                       (int)num_blocks, points, block_start, (int)V, density, gradient, color_sum);
  else
    hipLaunchKernelGGL((sample_eval_kernel<SAMPLE_PPT, false>), blocks, dim3(FIELD_THREADS), 0, st, prep.rec, prep.range, rgb, P,
                       (int)num_blocks, points, block_start, (int)V, density, gradient, color_sum);
  return hipGetLastError() == hipSuccess ? 0 : 3;
}
