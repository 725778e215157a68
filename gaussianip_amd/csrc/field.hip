// field.hip — leaving the Gaussian representation: the density field of a Gaussian set on a regular grid, and the iso-surface of
// a grid as an indexed triangle mesh.  Linked into libgip_model.so.  (gs_renderer.py:67-100 gaussian_3d_coeff, :240-331
// GaussianModel.extract_fields; the mesh of :333-361 is built by marching tetrahedra here, see below.)
//
// ---- density field -------------------------------------------------------------------------------------------------------------
// Definition (the reference's): the Gaussians that pass the opacity prefilter are normalised to xyz' = (xyz - center) * scale,
// std' = scaling * scale; Sigma = (R S)(R S)^T with R from the raw quaternion; the R^3 grid points are the outer product of `grid`
// (torch.linspace(-1, 1, R), computed by the caller), grouped in num_blocks^3 blocks of s = R / num_blocks points per axis.  A
// Gaussian belongs to a block when its centre lies STRICTLY inside the box [first - margin, last + margin] on all three axes (first /
// last = the block's first / last grid coordinate, margin = relax_ratio * 2 / num_blocks), and a voxel is the sum over its block's
// members of opacity * exp(power), power = -0.5 d^T Sigma^-1 d, a positive power counting as weight 0.  The cut is part of the
// definition, so everything that feeds it is written in the reference's operand order and this file is built with -ffp-contract=off.
//
//   field_prepare_kernel   one thread per Gaussian: xyz', the adjugate inverse of Sigma with 1 / (det + 1e-24), opacity -> a 10-float
//                          record; the per-axis interval of blocks the centre belongs to (lo[b] < x' and x' < hi[b] are monotone in
//                          b, so the members form one interval) -> one 64-bit word of six 10-bit fields, "empty" = first > last.
//                          The ONE prepare kernel of the field family: field_sample.hip and texture.hip launch it through
//                          field_prepare_launch, so membership and records are the same by construction.
//   field_eval_kernel      one workgroup per block, voxels on lanes (VPT voxels per lane, a further pass when a block has more than
//                          256 * 16).  Binning: NO duplicate list and NO sort — the walk of field_common.h (field_walk) over the P
//                          range words, which also evaluates the pairs; this kernel's own part is voxel -> point and address, and
//                          one sum per pair.
//
// ---- surface -------------------------------------------------------------------------------------------------------------------
// Marching tetrahedra on the Kuhn decomposition: every grid cube is cut into the six tetrahedra 0 -> e_a -> e_a + e_b -> (1,1,1), one
// per order (a, b, c) of the axes.  The cut is the same in every cube and the diagonal of a cube face is the same segment seen from
// both cubes, so neighbouring tetrahedra share whole faces and the surface is closed wherever it does not leave the grid.
// Every edge of every tetrahedron runs from a grid point p to p + d with d one of seven directions: a grid point owns seven edge
// slots (x, y, z, xy, xz, yz, xyz), edge id = point id * 7 + slot.  A crossing edge (exactly one end with f >= threshold) carries one
// vertex at t = (thr - f0) / (f1 - f0) from p.  Passes: flag crossing edges + count triangles per cube (gip_surface_count), two
// exclusive scans by the caller, vertices and faces (gip_surface_emit).  Vertex order = edge id, face order = cube id, tetrahedron,
// triangle of the case: deterministic.
#include "field_common.h"

#define FIELD_MAX_VPT 16

// ------------------------------------------------------------------------------------------------------------------ prepare
__global__ void __launch_bounds__(FIELD_THREADS)
field_prepare_kernel(const float* __restrict__ xyz, const float* __restrict__ opacity, const float* __restrict__ scaling,
                     const float* __restrict__ rotation, int64_t P, const float* __restrict__ center, float scale,
                     const float* __restrict__ grid, int R, int nb, float margin, float* __restrict__ rec, uint64_t* __restrict__ range) {
  const int64_t g = (int64_t)blockIdx.x * FIELD_THREADS + threadIdx.x;
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
  float* o = rec + g * FIELD_REC;
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

void field_prepare_launch(const float* xyz, const float* opacity, const float* scaling, const float* rotation, int64_t P,
                          const float* center, float scale, const float* grid, int R, int nb, float margin, FieldPrepared out,
                          hipStream_t stream) {
  hipLaunchKernelGGL(field_prepare_kernel, dim3((unsigned)((P + FIELD_THREADS - 1) / FIELD_THREADS)), dim3(FIELD_THREADS), 0, stream, xyz,
                     opacity, scaling, rotation, P, center, scale, grid, R, nb, margin, out.rec, out.range);
}

// ------------------------------------------------------------------------------------------------------------------ evaluate
template <int VPT>
__global__ void __launch_bounds__(FIELD_THREADS)
field_eval_kernel(const float* __restrict__ rec, const uint64_t* __restrict__ range, int64_t P, const float* __restrict__ grid, int R,
                  int nb, float* __restrict__ field) {
  __shared__ FieldLds<false> lds;
  const int tid = threadIdx.x;
  const int s = R / nb, s3 = s * s * s;
  const int bz = blockIdx.x % nb, by = (blockIdx.x / nb) % nb, bx = blockIdx.x / (nb * nb);

  for (int v0 = 0; v0 < s3; v0 += FIELD_THREADS * VPT) {      // one pass unless a block has more than 256 * 16 voxels
    float px[VPT], py[VPT], pz[VPT], acc[VPT][1];
    int64_t at[VPT];
#pragma unroll
    for (int k = 0; k < VPT; k++) {
      const int v = v0 + k * FIELD_THREADS + tid;
      const int vc = v < s3 ? v : 0;
      const int ix = bx * s + vc / (s * s), iy = by * s + (vc / s) % s, iz = bz * s + vc % s;
      px[k] = grid[ix];
      py[k] = grid[iy];
      pz[k] = grid[iz];
      at[k] = v < s3 ? ((int64_t)ix * R + iy) * R + iz : -1;
      acc[k][0] = 0.f;
    }
    field_walk<VPT, 1, false>(lds, rec, range, nullptr, P, bx, by, bz, px, py, pz, VPT, acc,
                              [](const FieldPair& q, float (&part)[1]) { part[0] = fmaf(q.c0.w, q.e, part[0]); });
#pragma unroll
    for (int k = 0; k < VPT; k++)
      if (at[k] >= 0) field[at[k]] = acc[k][0];
  }
}

extern "C" int gip_field_workspace_size(int64_t P, int32_t R, int32_t num_blocks, size_t* bytes) {
  return field_workspace_size(P, R, num_blocks, bytes);
}

extern "C" int gip_density_field(const float* xyz, const float* opacity, const float* scaling, const float* rotation, int64_t P,
                                 const float* center, float scale, const float* grid, int32_t R, int32_t num_blocks, float margin,
                                 void* workspace, size_t workspace_bytes, float* field, void* stream) {
  size_t need = 0;
  if (field_workspace_size(P, R, num_blocks, &need) != 0 || !grid || !field) return 1;
  if (P > 0 && (!xyz || !opacity || !scaling || !rotation || !center || !workspace || workspace_bytes < need)) return 1;
  const int s = R / num_blocks;
  const int64_t s3 = (int64_t)s * s * s;
  if (s3 > INT32_MAX) return 1;
  const FieldPrepared prep = field_workspace_split(workspace, P);
  hipStream_t st = (hipStream_t)stream;
  if (P > 0) field_prepare_launch(xyz, opacity, scaling, rotation, P, center, scale, grid, (int)R, (int)num_blocks, margin, prep, st);
  const dim3 blocks((unsigned)(num_blocks * num_blocks * num_blocks));
#define FIELD_LAUNCH(V) \
  hipLaunchKernelGGL(field_eval_kernel<V>, blocks, dim3(FIELD_THREADS), 0, st, prep.rec, prep.range, P, grid, (int)R, (int)num_blocks, field)
  if (s3 <= FIELD_THREADS) FIELD_LAUNCH(1);
  else if (s3 <= 2 * FIELD_THREADS) FIELD_LAUNCH(2);
  else if (s3 <= 4 * FIELD_THREADS) FIELD_LAUNCH(4);
  else if (s3 <= 8 * FIELD_THREADS) FIELD_LAUNCH(8);
  else FIELD_LAUNCH(FIELD_MAX_VPT);
#undef FIELD_LAUNCH
  return hipGetLastError() == hipSuccess ? 0 : 3;
}

// ------------------------------------------------------------------------------------------------------------------ surface
// The six Kuhn tetrahedra as cube corners (bit 0 = +x, bit 1 = +y, bit 2 = +z), axis orders xyz, xzy, yxz, yzx, zxy, zyx.  With corners
// (v0, v1, v2, v3) = (0, e_a, e_a + e_b, 7), det(v1 - v0, v2 - v0, v3 - v0) is the sign of the permutation; the odd orders are listed
// with v1 and v2 exchanged, so that EVERY row is positively oriented and one case table serves all six.
__constant__ uint8_t kTetCorner[6][4] = {{0, 1, 3, 7}, {0, 5, 1, 7}, {0, 3, 2, 7}, {0, 2, 6, 7}, {0, 4, 5, 7}, {0, 6, 4, 7}};
// edge slot of a direction mask: x, y, z, xy, xz, yz, xyz
__constant__ int8_t kSlot[8] = {-1, 0, 1, 3, 2, 4, 5, 6};

// Case table of a positively oriented tetrahedron (0, 1, 2, 3); bit i of the case = corner i inside (f >= thr).  An entry `ab` is the
// vertex on the edge between corners a and b (two octal digits).  Derivation, with (a, b, c, d) an EVEN permutation of (0, 1, 2, 3):
//   one corner a inside: triangle (ab, ac, ad).  Put a at the origin, u_b = b - a ...: det(u_b, u_c, u_d) > 0 for an even permutation
//       of a positively oriented tetrahedron, the triangle's normal n = (P_ac - P_ab) x (P_ad - P_ab) has n . (a - P_ab) =
//       -t_b t_c t_d det(u_b, u_c, u_d) < 0: the inside corner is behind the triangle, the normal points to decreasing density.
//   one corner a outside: the same triangle seen from the other side: (ab, ad, ac).
//   corners a, b inside: let b sink below the threshold from the one-inside case: the vertex ab of the cycle ac -> ad -> ab splits
//       into bd (next to ad on face a b d) and bc (next to ac on face a b c): the cycle ac -> ad -> bd -> bc, cut along ac - bd.
__constant__ uint8_t kTetCase[16][7] = {
    {0, 0, 0, 0, 0, 0, 0},                 // ....  nothing inside
    {1, 001, 002, 003, 0, 0, 0},           // 0     (a b c d) = (0 1 2 3)
    {1, 010, 013, 012, 0, 0, 0},           // 1     (1 0 3 2)
    {2, 002, 003, 013, 002, 013, 012},     // 0 1   (0 1 2 3): 02 -> 03 -> 13 -> 12
    {1, 020, 021, 023, 0, 0, 0},           // 2     (2 0 1 3)
    {2, 003, 001, 021, 003, 021, 023},     // 0 2   (0 2 3 1): 03 -> 01 -> 21 -> 23
    {2, 010, 013, 023, 010, 023, 020},     // 1 2   (1 2 0 3): 10 -> 13 -> 23 -> 20
    {1, 030, 031, 032, 0, 0, 0},           // 0 1 2 corner 3 outside, (3 0 2 1) even: (30, 31, 32) = (ab, ad, ac)
    {1, 030, 032, 031, 0, 0, 0},           // 3     (3 0 2 1)
    {2, 001, 002, 032, 001, 032, 031},     // 0 3   (0 3 1 2): 01 -> 02 -> 32 -> 31
    {2, 012, 010, 030, 012, 030, 032},     // 1 3   (1 3 2 0): 12 -> 10 -> 30 -> 32
    {1, 020, 023, 021, 0, 0, 0},           // 0 1 3 corner 2 outside, (2 0 1 3): (20, 23, 21)
    {2, 020, 021, 031, 020, 031, 030},     // 2 3   (2 3 0 1): 20 -> 21 -> 31 -> 30
    {1, 010, 012, 013, 0, 0, 0},           // 0 2 3 corner 1 outside, (1 0 3 2): (10, 12, 13)
    {1, 001, 003, 002, 0, 0, 0},           // 1 2 3 corner 0 outside, (0 1 2 3): (01, 03, 02)
    {0, 0, 0, 0, 0, 0, 0}};                // everything inside

__device__ __forceinline__ int surface_case(const float* __restrict__ field, int R, int i, int j, int k, int tet, float thr) {
  int m = 0;
#pragma unroll
  for (int c = 0; c < 4; c++) {
    const int cm = kTetCorner[tet][c];
    const float f = field[((int64_t)(i + (cm & 1)) * R + (j + ((cm >> 1) & 1))) * R + (k + ((cm >> 2) & 1))];
    m |= (f >= thr ? 1 : 0) << c;
  }
  return m;
}

// one thread per grid point: its seven edge flags; and, when the point is the origin of a cube, that cube's triangle count
__global__ void __launch_bounds__(256)
surface_count_kernel(const float* __restrict__ field, int R, float thr, int32_t* __restrict__ edge_flag, int32_t* __restrict__ tri_count) {
  const int64_t pt = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (pt >= (int64_t)R * R * R) return;
  const int k = (int)(pt % R), j = (int)((pt / R) % R), i = (int)(pt / ((int64_t)R * R));
  const bool in0 = field[pt] >= thr;
#pragma unroll
  for (int d = 1; d < 8; d++) {
    const int i1 = i + (d & 1), j1 = j + ((d >> 1) & 1), k1 = k + ((d >> 2) & 1);
    int flag = 0;
    if (i1 < R && j1 < R && k1 < R) flag = (field[((int64_t)i1 * R + j1) * R + k1] >= thr) != in0;
    edge_flag[pt * 7 + kSlot[d]] = flag;
  }
  if (i < R - 1 && j < R - 1 && k < R - 1) {
    int n = 0;
    for (int t = 0; t < 6; t++) n += kTetCase[surface_case(field, R, i, j, k, t, thr)][0];
    tri_count[((int64_t)i * (R - 1) + j) * (R - 1) + k] = n;
  }
}

__global__ void __launch_bounds__(256)
surface_emit_kernel(const float* __restrict__ field, int R, float thr, const int32_t* __restrict__ edge_flag,
                    const int32_t* __restrict__ edge_index, const int32_t* __restrict__ tri_offset, float* __restrict__ vertices,
                    int32_t* __restrict__ faces) {
  const int64_t pt = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (pt >= (int64_t)R * R * R) return;
  const int k = (int)(pt % R), j = (int)((pt / R) % R), i = (int)(pt / ((int64_t)R * R));
  const float f0 = field[pt];
#pragma unroll
  for (int d = 1; d < 8; d++) {
    const int64_t e = pt * 7 + kSlot[d];
    if (!edge_flag[e]) continue;
    const int di = d & 1, dj = (d >> 1) & 1, dk = (d >> 2) & 1;
    const float f1 = field[((int64_t)(i + di) * R + (j + dj)) * R + (k + dk)];
    const float t = (thr - f0) / (f1 - f0);   // the ends lie on different sides of thr: f1 != f0
    float* v = vertices + (int64_t)edge_index[e] * 3;
    v[0] = (float)i + t * (float)di;
    v[1] = (float)j + t * (float)dj;
    v[2] = (float)k + t * (float)dk;
  }
  if (i >= R - 1 || j >= R - 1 || k >= R - 1) return;
  int32_t* out = faces + (int64_t)tri_offset[((int64_t)i * (R - 1) + j) * (R - 1) + k] * 3;
  for (int t = 0; t < 6; t++) {
    const uint8_t* cs = kTetCase[surface_case(field, R, i, j, k, t, thr)];
    for (int n = 0; n < 3 * cs[0]; n++) {
      const int ca = kTetCorner[t][cs[1 + n] >> 3], cb = kTetCorner[t][cs[1 + n] & 7];
      const int lo = ca & cb, d = ca ^ cb;   // along a Kuhn edge one corner's offsets contain the other's
      const int64_t p = ((int64_t)(i + (lo & 1)) * R + (j + ((lo >> 1) & 1))) * R + (k + ((lo >> 2) & 1));
      *out++ = edge_index[p * 7 + kSlot[d]];
    }
  }
}

static int surface_shape_ok(int32_t R) { return R >= 2 && (int64_t)R * R * R * 7 <= INT32_MAX; }

extern "C" int gip_surface_count(const float* field, int32_t R, float threshold, int32_t* edge_flag, int32_t* tri_count, void* stream) {
  if (!field || !edge_flag || !tri_count || !surface_shape_ok(R)) return 1;
  const int64_t pts = (int64_t)R * R * R;
  hipLaunchKernelGGL(surface_count_kernel, dim3((unsigned)((pts + 255) / 256)), dim3(256), 0, (hipStream_t)stream, field, (int)R, threshold,
                     edge_flag, tri_count);
  return hipGetLastError() == hipSuccess ? 0 : 3;
}

extern "C" int gip_surface_emit(const float* field, int32_t R, float threshold, const int32_t* edge_flag, const int32_t* edge_index,
                                const int32_t* tri_offset, float* vertices, int32_t* faces, void* stream) {
  if (!field || !edge_flag || !edge_index || !tri_offset || !vertices || !faces || !surface_shape_ok(R)) return 1;
  const int64_t pts = (int64_t)R * R * R;
  hipLaunchKernelGGL(surface_emit_kernel, dim3((unsigned)((pts + 255) / 256)), dim3(256), 0, (hipStream_t)stream, field, (int)R, threshold,
                     edge_flag, edge_index, tri_offset, vertices, faces);
  return hipGetLastError() == hipSuccess ? 0 : 3;
}
