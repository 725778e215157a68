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
// The Gaussians are prepared by field.hip's kernel (field_prepare_launch): the same records and range words, so membership is
// gip_density_field's.
//   texture_eval_kernel     grid = block x slice.  A block's texel slots ((faces of the block) * cell (cell + 1) / 2; slot -> (li, lj)
//                           by folding the triangle's rows r and cell - r [cell odd] or cell - 1 - r [cell even] into one row of a
//                           rectangle; the odd face skips the cell slots of the diagonal li + lj = cell - 1, which half 0 owns) are cut
//                           into passes of 256 * PPT; slice s takes passes s, s + slices, ...  A workgroup whose first pass lies
//                           past the block's count returns before it reads a range word.  A lane derives its texels' faces, local
//                           indices and points in registers: no point array is read, and the sums go straight into the texture.
//                           Members are found and pairs evaluated by the walk that sample_eval_kernel uses (field_common.h:
//                           field_walk): given the same points and blocks the sums are gip_field_sample's bit for bit, whatever
//                           `slices` is.  Only density and colour are accumulated: 3 + 4 + 4 registers per point.
#include "field_common.h"

#define TEX_PPT 4                               // texels per lane and pass: 4 sums + 4 batch sums + 3 coordinates each
#define TEX_PASS (FIELD_THREADS * TEX_PPT)      // texel slots of one pass
#define TEX_MAX_SIZE 16384
#define TEX_MAX_SLICES 65535                    // the grid's second dimension
#define TEX_AUTO_SLICES 1024

template <int PPT>
__global__ void __launch_bounds__(FIELD_THREADS)
texture_eval_kernel(const float* __restrict__ rec, const uint64_t* __restrict__ range, const float* __restrict__ rgb, int64_t P, int nb,
                    const float* __restrict__ vertices, int V, const int32_t* __restrict__ faces, int F,
                    const int32_t* __restrict__ face_order, const int32_t* __restrict__ block_start, int T, int cell,
                    float* __restrict__ density, float* __restrict__ color_sum) {
  // the block's faces; clipped to [0, F] so that no offset, whatever the caller wrote there, leads outside the arrays
  const int first = max(block_start[blockIdx.x], 0), end = min(block_start[blockIdx.x + 1], F);
  if (end <= first) return;   // no face here: not a single range word is read
  const int per_face = cell * (cell + 1) / 2;
  const int total = (end - first) * per_face;   // < 2^31: F * per_face <= (T / cell)^2 * cell * (cell + 1) <= 1.25 T^2
  if ((int64_t)blockIdx.y * (FIELD_THREADS * PPT) >= total) return;   // this slice has no pass: nothing read either
  __shared__ FieldLds<true> lds;
  const int tid = threadIdx.x;
  const int bz = blockIdx.x % nb, by = (blockIdx.x / nb) % nb, bx = blockIdx.x / (nb * nb);
  const int n = T / cell, leg = cell - 3, fold = cell | 1;    // fold: the width of the rectangle the triangle's rows are folded into
  const float fleg = (float)leg;

  for (int p0 = (int)blockIdx.y * (FIELD_THREADS * PPT); p0 < total; p0 += (int)gridDim.y * (FIELD_THREADS * PPT)) {
    const int slots = (min(total - p0, FIELD_THREADS * PPT) + FIELD_THREADS - 1) / FIELD_THREADS;   // slots in use: workgroup-uniform
    float px[PPT], py[PPT], pz[PPT], acc[PPT][4];
    int at[PPT];
#pragma unroll
    for (int k = 0; k < PPT; k++) {
      const int t = p0 + k * FIELD_THREADS + tid;
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
    field_walk<PPT, 4, true>(lds, rec, range, rgb, P, bx, by, bz, px, py, pz, slots, acc, [](const FieldPair& q, float (&part)[4]) {
      part[0] = fmaf(q.c0.w, q.e, part[0]);
      const float w = q.c0.w * q.e;
      part[1] = fmaf(w, q.c3.x, part[1]);
      part[2] = fmaf(w, q.c3.y, part[2]);
      part[3] = fmaf(w, q.c3.z, part[3]);
    });
#pragma unroll
    for (int k = 0; k < PPT; k++) {
      if (at[k] < 0) continue;
      const int64_t o = at[k];
      density[o] = acc[k][0];
      color_sum[o * 3] = acc[k][1];
      color_sum[o * 3 + 1] = acc[k][2];
      color_sum[o * 3 + 2] = acc[k][3];
    }
  }
}

extern "C" int gip_texture_bake_workspace_size(int64_t P, int32_t R, int32_t num_blocks, size_t* bytes) {
  return field_workspace_size(P, R, num_blocks, bytes);
}

extern "C" int gip_texture_bake(const float* xyz, const float* opacity, const float* scaling, const float* rotation, const float* rgb,
                                int64_t P, const float* center, float scale, const float* grid, int32_t R, int32_t num_blocks,
                                float margin, const float* vertices, int64_t V, const int32_t* faces, int64_t F,
                                const int32_t* face_order, const int32_t* block_start, int32_t T, int32_t cell, int32_t slices,
                                void* workspace, size_t workspace_bytes, float* density, float* color_sum, void* stream) {
  size_t need = 0;
  if (field_workspace_size(P, R, num_blocks, &need) != 0) return 1;
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
  const FieldPrepared prep = field_workspace_split(workspace, P);
  field_prepare_launch(xyz, opacity, scaling, rotation, P, center, scale, grid, (int)R, (int)num_blocks, margin, prep, st);
  const dim3 blocks((unsigned)(num_blocks * num_blocks * num_blocks), (unsigned)slices);
  hipLaunchKernelGGL((texture_eval_kernel<TEX_PPT>), blocks, dim3(FIELD_THREADS), 0, st, prep.rec, prep.range, rgb, P, (int)num_blocks,
                     vertices, (int)V, faces, (int)F, face_order, block_start, (int)T, (int)cell, density, color_sum);
  return hipGetLastError() == hipSuccess ? 0 : 3;
}
