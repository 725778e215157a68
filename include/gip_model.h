/*
 * gip_model.h — C-ABI of the device-side Gaussian-set surgery used by densify / prune.
 *
 *   gip_gather_rows  <->  the chain of boolean-mask indexing and torch.cat calls that rebuilds the six parameter
 *       tensors and their twelve Adam moment tensors whenever the reference densifies or prunes
 *       (gaussiansplatting/scene/gaussian_model.py:292-355 prune_points / cat_tensors_to_optimizer /
 *       densification_postfix, driven by densify_and_prune :395-411 and prune_only :413-418).
 *
 * The final row order of clone -> split -> prune is fully described by one index list over the virtual concatenation
 * [old rows | new rows]; every tensor is then rebuilt by ONE gather, all tensors in ONE launch:
 *       dst_t[j] = index[j] < n_old ? old_t[index[j]] : (new_t ? new_t[index[j] - n_old] : 0)
 * (new_t == NULL writes zero rows: the Adam moments of freshly created Gaussians).  Byte-exact data movement: rows
 * are copied as 4-byte words, row_bytes % 4 == 0.  Plain C, raw device pointers, caller-owned buffers, work enqueued
 * on `stream`, integer status (0 ok, 1 bad argument, 3 HIP error).  `tensors` is a HOST array (at most 24 entries).
 */
#ifndef GIP_MODEL_H
#define GIP_MODEL_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define GIP_GATHER_MAX_TENSORS 24
typedef struct {
  const void* old_rows; /* [n_old, row_bytes] device */
  const void* new_rows; /* [n_new, row_bytes] device, or NULL for zero rows */
  void* dst;            /* [n_out, row_bytes] device */
  int32_t row_bytes;
  int32_t reserved;
} GipGatherTensor;
int gip_gather_rows(const GipGatherTensor* tensors, int32_t n_tensors, const int64_t* index /* [n_out] device */,
                    int64_t n_out, int64_t n_old, void* stream);

/* Bucket packing for the per-step multi-GPU exchange (gaussianip_amd/parallel.py; SURVEY.md §8e: all_reduce(sum) of the
 * six parameter gradients and of the per-Gaussian view-space gradient norms that GaussianIP.py:452-457 accumulates):
 *   gip_pack_bucket    flat = [seg_0 | seg_1 | ... | tail], tail[p] = sum_v sqrt(g2d[v,p,0]^2 + g2d[v,p,1]^2) when g2d is
 *                      given (g2d [V, P, 3] float, the means2D gradients of the local views; tail has P floats), in ONE
 *                      launch instead of a norm, a sum and a concatenation;
 *   gip_unpack_bucket  seg_i <- flat[offset_i : offset_i + n_i] * scale (scale = 1 / world for averaged gradients), and
 *                      tail_dst <- flat tail (unscaled) when given, in one launch.
 * Segments are float32 device arrays (at most GIP_PACK_MAX_SEGS), `segs` / `counts` are HOST arrays. */
#define GIP_PACK_MAX_SEGS 12
int gip_pack_bucket(const void* const* segs, const int64_t* counts, int32_t n_segs, const void* g2d, int32_t V, int64_t P,
                    void* flat, void* stream);
int gip_unpack_bucket(void* const* segs, const int64_t* counts, int32_t n_segs, void* tail_dst, int64_t tail_count,
                      const void* flat, float scale, void* stream);

/* The MAX bucket of the same exchange (GaussianIP.py:225 batch-global depth maximum, :452-457 max_radii2D), straight
 * from the rasterizer's forward outputs in one launch:
 *   out[p] = max_v radii[v, p]  (p < P, int32),   out[P] = bit pattern of max(depth[0 .. n_depth))  (float32 >= 0:
 *   non-negative IEEE floats order like their bit patterns, so an int32 all_reduce(max) of the whole bucket is exact). */
int gip_max_bucket(const int32_t* radii, int32_t V, int64_t P, const float* depth, int64_t n_depth, int32_t* out, void* stream);

/* One Adam step for ALL parameter groups of the Gaussian model in ONE launch (torch.optim.Adam, no weight decay, no amsgrad;
 * gaussiansplatting/scene/gaussian_model.py:145-155 builds six single-tensor groups with their own learning rates, eps 1e-15).
 * torch's fused Adam launches three multi-tensor kernels per group (18 launches, 0.29 ms of a 39 ms step for 5.6 MB of state).
 *   step_t += 1;  m = m + (1 - beta1) (g - m);  v = beta2 v + (1 - beta2) g^2;
 *   p -= lr / (1 - beta1^t) * (m / (sqrt(v) / sqrt(1 - beta2^t) + eps))        (torch.optim.Adam's operation order; the bias
 *   corrections and 1 - beta in double arithmetic like torch's Python-side constants)
 * `step` of every group is a device float scalar (torch's own state["step"] of a fused / capturable Adam) and is incremented by
 * the kernel.  found_inf (device float, may be NULL): a GradScaler's verdict — when non-zero nothing is written (the skipped
 * step of torch.amp; the gradients were unscaled before).  `groups` is a HOST array (at most GIP_ADAM_MAX_GROUPS). */
#define GIP_ADAM_MAX_GROUPS 8
typedef struct {
  void* param;        /* [n] float32 device */
  const void* grad;   /* [n] float32 device */
  void* exp_avg;      /* [n] float32 device */
  void* exp_avg_sq;   /* [n] float32 device */
  float* step;        /* device scalar */
  int64_t n;
  float lr;
  int32_t reserved;
} GipAdamGroup;
int gip_adam_step(const GipAdamGroup* groups, int32_t n_groups, double beta1, double beta2, double eps, const float* found_inf,
                  void* stream);   /* betas / eps as doubles: the caller's Python floats, no re-rounding (0 <= beta < 1, else status 1) */

/* The sparsity term of the stage-1 loss (threestudio/systems/GaussianIP.py:225, :377-380):
 *   mean(sqrt((depth / (max(depth) + 1e-5))^2 + 0.01))   over the n = B * H * W depths of a step,
 * three launches forward, two backward (the reference's op chain: ~20 launches on 4 M elements), fixed summation orders.
 * workspace: gip_sparsity_workspace_bytes() bytes, kept between forward and backward;
 * after forward: ((float*)workspace)[0] = max(depth), [1] = the term.  backward: g_depth[i] = d term / d depth[i] * g_loss[0] * mult
 * (the maximum's share through the denominator goes evenly to the elements equal to it, like torch.max()'s backward). */
size_t gip_sparsity_workspace_bytes(void);
int gip_sparsity_loss_forward(const float* depth, int64_t n, void* workspace, void* stream);
int gip_sparsity_loss_backward(const float* depth, int64_t n, const float* g_loss, float mult, void* workspace, float* g_depth,
                               void* stream);

/* The three parameter activations of GaussianModel (gaussiansplatting/scene/gaussian_model.py:36-41, getters :72-89) in one launch:
 *   opacity [P] = sigmoid(opacity_raw), scaling [P,3] = exp(scaling_raw), rotation [P,4] = rotation_raw / max(||rotation_raw||, 1e-12)
 * (float32, contiguous), and their backward in one launch (g_* may be NULL = no gradient arrived for that output; d_* may be NULL). */
int gip_activate_gaussians(const float* opacity_raw, const float* scaling_raw, const float* rotation_raw, int64_t P, float* opacity,
                           float* scaling, float* rotation, void* stream);
int gip_activate_gaussians_backward(const float* opacity, const float* scaling, const float* rotation_raw, const float* g_opacity,
                                    const float* g_scaling, const float* g_rotation, int64_t P, float* d_opacity_raw,
                                    float* d_scaling_raw, float* d_rotation_raw, void* stream);

/* Densification statistics of one step in one launch (threestudio/systems/GaussianIP.py:451-457, gaussian_model.py:420-422):
 *   grad = sum over the V views of viewspace_grad [V,P,3];  where visible: max_radii2D = max(max_radii2D, radii);
 *   xyz_gradient_accum += ||grad[:, :2]|| * visible;  denom += visible.   (visible: bytes 0 / 1; radii int32; the rest float32 [P].) */
int gip_densify_stats(const float* viewspace_grad, int32_t V, int64_t P, const uint8_t* visible, const int32_t* radii,
                      float* max_radii2D, float* xyz_gradient_accum, float* denom, void* stream);

/* The structural-similarity loss of the 3DGS trainers (gaussiansplatting/utils/loss_utils.py:33-63 ssim / _ssim; the window of
 * :23-31): an 11 x 11 Gaussian window (sigma 1.5, normalised in float32) with zero padding of 5 pixels, depthwise on
 * [N, C, H, W] float32 contiguous images, C1 = 0.01^2, C2 = 0.03^2.  One tiled kernel forward (+ a one-workgroup-per-image pass
 * that adds the per-workgroup partial sums in a fixed order: no float atomics, bitwise reproducible) and one backward, instead of
 * five grouped 121-tap convolutions, a dozen pointwise ops and their autograd graph.
 *   gip_ssim_workspace_bytes  bytes of `workspace` for a shape (0 for a shape the entry points reject);
 *   gip_ssim_forward   per_image_mean[n] = mean over (c, h, w) of the SSIM map of image n  (loss_utils.py:63; their mean is :61).
 *                      deriv (or NULL: nothing but the means is written) receives [3, N, C, H, W]: the three planes the backward
 *                      needs (d m / d mu1 with the variance terms folded in, d m / d sigma1^2, d m / d sigma12);
 *                      map (or NULL) receives the SSIM map [N, C, H, W];
 *   gip_ssim_backward  g_img1 = sum_n g_per_image[n] * d per_image_mean[n] / d img1   ([N, C, H, W]); g_per_image is a DEVICE
 *                      array of N floats, so no host synchronisation enters a training step.  img2 is data: no gradient.
 * Status 1: an empty or negative dimension, a NULL required pointer, more than 2^31 - 1 tiles of 32 x 32. */
size_t gip_ssim_workspace_bytes(int32_t N, int32_t C, int32_t H, int32_t W);
int gip_ssim_forward(const float* img1, const float* img2, int32_t N, int32_t C, int32_t H, int32_t W, float* per_image_mean,
                     float* deriv, float* map, void* workspace, void* stream);
int gip_ssim_backward(const float* img1, const float* img2, const float* deriv, const float* g_per_image, int32_t N, int32_t C,
                      int32_t H, int32_t W, float* g_img1, void* stream);
/* Leaving the Gaussian representation (gs_renderer.py:67-100 gaussian_3d_coeff, :240-331 GaussianModel.extract_fields; csrc/field.hip).
 *   gip_density_field  field[i, j, k] ([R, R, R] float32, `ij` order) = sum over the members of the voxel's block of
 *       opacity * exp(-0.5 d^T Sigma^-1 d), d = (grid[i], grid[j], grid[k]) - xyz', xyz' = (xyz - center) * scale, Sigma from
 *       scaling * scale and the raw quaternion, inverted by the adjugate with 1 / (det + 1e-24); a positive power counts as 0.
 *       The grid points are grouped in num_blocks^3 blocks (R % num_blocks == 0, num_blocks <= 1024); a Gaussian is a member of a
 *       block when xyz' lies strictly inside [first - margin, last + margin] of the block's grid coordinates on all three axes
 *       (margin = relax_ratio * 2 / num_blocks rounded to float32); blocks without a member are exactly 0.
 *       The caller passes the P Gaussians that passed its prefilter (P = 0 gives zeros): xyz [P, 3], activated opacity [P], activated
 *       scaling [P, 3], raw rotation [P, 4], center [3] (device), grid [R] (device; torch.linspace(-1, 1, R), not re-derived here).
 *       Members are added in the order of the arrays, no float atomics: two runs are bitwise equal.  No host read.
 *   gip_field_workspace_size  bytes of `workspace` (a record and a block-range word per Gaussian).
 *   gip_surface_count / gip_surface_emit  the iso-surface f = threshold of any [R, R, R] float32 grid as an indexed triangle mesh
 *       (marching tetrahedra on the Kuhn decomposition; a grid point is inside when f >= threshold; normals toward decreasing f;
 *       open where the surface leaves the grid).  count: edge_flag [R^3 * 7] int32 (1 = the edge carries a vertex; edge id =
 *       point id * 7 + slot, slots x, y, z, xy, xz, yz, xyz) and tri_count [(R - 1)^3] int32 (triangles of each cube).  The caller
 *       scans both exclusively (edge_index, tri_offset), reads the two totals V and F, allocates vertices [V, 3] float32 (grid-index
 *       units) and faces [F, 3] int32, and calls emit.  Vertex order = edge id, face order = cube id, tetrahedron: deterministic.
 * Status 1: a NULL required pointer, a shape outside the limits (R < 2 or 7 R^3 > 2^31 - 1 for the surface), a short workspace. */
int gip_field_workspace_size(int64_t P, int32_t R, int32_t num_blocks, size_t* bytes);
int gip_density_field(const float* xyz, const float* opacity, const float* scaling, const float* rotation, int64_t P,
                      const float* center, float scale, const float* grid, int32_t R, int32_t num_blocks, float margin,
                      void* workspace, size_t workspace_bytes, float* field, void* stream);
int gip_surface_count(const float* field, int32_t R, float threshold, int32_t* edge_flag, int32_t* tri_count, void* stream);
int gip_surface_emit(const float* field, int32_t R, float threshold, const int32_t* edge_flag, const int32_t* edge_index,
                     const int32_t* tri_offset, float* vertices, int32_t* faces, void* stream);
/* The same field asked for at arbitrary points (csrc/field_sample.hip): vertex colours and analytic normals of the mesh above.
 *   gip_field_sample  for each of V query points, given in NORMALISED coordinates and grouped by the block they are evaluated in
 *       (points [V, 3]; block_start [num_blocks^3 + 1] int32 exclusive offsets into points, block id = (bx * nb + by) * nb + bz;
 *       the CALLER decides a point's block), the sums over that block's members of
 *           density   [V]     sum w,              w = opacity * exp(-0.5 d^T Sigma^-1 d), d = x - xyz', a positive power counting as 0
 *           gradient  [V, 3]  sum w * (-Sigma^-1 d)   (the gradient of the density in normalised space; or NULL)
 *           color_sum [V, 3]  sum w * rgb             (raw: dividing by density is the caller's; or NULL, rgb [P, 3] may then be NULL)
 *       Sources, normalisation, inverse covariance, blocks, membership and `margin` are gip_density_field's, argument for argument;
 *       at a grid point evaluated in its own block, density is bit for bit that voxel of gip_density_field.  A block without points
 *       costs nothing but its launch; members are added in the order of the arrays, no float atomics: two runs are bitwise equal.
 *       V == 0 is a successful no-op; P == 0 fills the outputs with zeros.  No host read.
 *   gip_field_sample_workspace_size  bytes of `workspace` (a record and a block-range word per Gaussian).
 * Status 1: a NULL required pointer, a shape outside gip_density_field's limits, V > 2^31 - 1, a short workspace, rgb == NULL while
 * color_sum != NULL. */
int gip_field_sample_workspace_size(int64_t P, int32_t R, int32_t num_blocks, size_t* bytes);
int gip_field_sample(const float* xyz, const float* opacity, const float* scaling, const float* rotation, const float* rgb, int64_t P,
                     const float* center, float scale, const float* grid, int32_t R, int32_t num_blocks, float margin,
                     const float* points, const int32_t* block_start, int64_t V, void* workspace, size_t workspace_bytes,
                     float* density, float* gradient, float* color_sum, void* stream);
/* The colour of the Gaussians baked into a UV texture of a triangle mesh (csrc/texture.hip; the atlas is stated in
 * gaussianip_amd/utils/texture.py): face f owns a right-isosceles triangle of texels, half f & 1 of the cell x cell square f / 2
 * (row-major, T / cell squares per row; a texel with cell-local indices (i, j) belongs to half (i + j >= cell)).
 *   gip_texture_bake  for every owned texel of a T x T texture (row 0 = the top image row), at the point
 *           p = v0 + (li / b) (v1 - v0) + (lj / b) (v2 - v0),   b = cell - 3,   (li, lj) = (i, j) or (cell - 1 - i, cell - 1 - j) for half 1,
 *       of its face (float32, that operand order; vertices [V, 3] in NORMALISED coordinates, faces [F, 3] int32), the sums over the
 *       members of the face's block of
 *           density   [T, T]     sum w            color_sum [T, T, 3]  sum w * rgb        (w as in gip_field_sample; raw sums)
 *       The CALLER decides a face's block: face_order [F] int32 lists the face ids grouped by block, block_start [num_blocks^3 + 1]
 *       int32 are the exclusive offsets into it.  Sources, normalisation, inverse covariance, blocks, membership and `margin` are
 *       gip_density_field's, argument for argument; the walk over the Gaussians is gip_field_sample's, so the sums equal
 *       gip_field_sample's at the same points and blocks bit for bit.  A block's texels are spread over `slices` workgroups (0: chosen
 *       here from F alone; the result does not depend on it); no float atomics: two runs are bitwise equal.  Unowned texels are not
 *       written: the caller zero-fills.  F == 0 is a successful no-op; P == 0 fills both outputs with zeros.  No host read.
 *   gip_texture_bake_workspace_size  bytes of `workspace` (gip_field_sample_workspace_size's).
 * Status 1: a NULL required pointer, a shape outside gip_density_field's limits, T < 4 or T > 16384, cell < 4, cell > T or
 * 2 (T / cell)^2 < F, slices < 0 or > 65535, a short workspace, F or V above 2^31 - 1, faces without vertices.  Status 3: a launch error. */
int gip_texture_bake_workspace_size(int64_t P, int32_t R, int32_t num_blocks, size_t* bytes);
int gip_texture_bake(const float* xyz, const float* opacity, const float* scaling, const float* rotation, const float* rgb, int64_t P,
                     const float* center, float scale, const float* grid, int32_t R, int32_t num_blocks, float margin,
                     const float* vertices, int64_t V, const int32_t* faces, int64_t F, const int32_t* face_order,
                     const int32_t* block_start, int32_t T, int32_t cell, int32_t slices, void* workspace, size_t workspace_bytes,
                     float* density, float* color_sum, void* stream);
/* Rendered views projected onto the same atlas (csrc/texture_project.hip, whose header states the definition with its float32
 * operand order): the other source of a texture's colours, what a camera sees instead of the field's volumetric blend.
 *   gip_texture_project  for every owned texel of a T x T texture, at the point p of gip_texture_bake's formula on vertices [V, 3] in
 *       WORLD coordinates (faces [F, 3] int32), and for the views k = 0 .. K - 1 in that order (1 <= K <= 64; views [K, 20]: the
 *       camera's full_proj_transform, 16 values in the row-vector convention clip = (p, 1) M, its camera_center, one pad):
 *           skip unless clip w > 0;   (sx, sy) = ((x / w) 0.5 + 0.5) W, ((y / w) 0.5 + 0.5) H, pixel (ix, iy) has its centre at
 *           (ix + 0.5, iy + 0.5);   skip unless 0 <= sx < W and 0 <= sy < H;   wp = vis_depth[k, floor(sy), floor(sx)] (vis_depth
 *           [K, H, W]: the clip w of the mesh surface visible at each pixel centre, <= 0 where nothing is drawn): skip unless wp > 0
 *           and w - wp <= depth_tolerance;   cos of the angle between the face's normal (v1 - v0) x (v2 - v0) and camera_center - p,
 *           its absolute value when two_sided: skip unless cos >= min_cos (a face with a zero normal contributes nothing);   the
 *           bilinear lookup of images[k] ([K, H, W, 4] interleaved r, g, b, a; 16-byte aligned) at (sx - 0.5, sy - 0.5), indices
 *           clamped: skip unless a >= min_alpha;   unpremultiply: rgb / a;
 *           weight_sum [T, T] += cos^2     color_sum [T, T, 3] += cos^2 * rgb     count [T, T] int32 += 1
 *       Owned texels are written (zeros when no view passes), unowned ones are not: the caller zero-fills all three.  One lane per
 *       texel, no atomics: two runs are bitwise equal.  F == 0 is a successful no-op.  No workspace, no host read.
 * Status 1: K outside 1 .. 64, T < 4 or T > 16384, cell < 4, cell > T or 2 (T / cell)^2 < F, H or W outside 1 .. 16384, F or V above
 * 2^31 - 1, a NULL pointer, faces without vertices, images not 16-byte aligned, unpremultiply with min_alpha <= 0.  Status 3: a
 * launch error. */
int gip_texture_project(const float* vertices, int64_t V, const int32_t* faces, int64_t F, int32_t T, int32_t cell, int32_t K,
                        const float* views, const float* images, const float* vis_depth, int32_t H, int32_t W, float depth_tolerance,
                        float min_cos, float min_alpha, int32_t two_sided, int32_t unpremultiply, float* color_sum, float* weight_sum,
                        int32_t* count, void* stream);
/* Rendering the textured mesh (csrc/mesh_raster.hip, whose header states the definition of coverage, visibility, interpolation and
 * lookup; gaussianip_amd/utils/rasterize.py).  All tensors float32 and contiguous, indices int32, everything on the device.
 *   gip_mesh_rasterize  pos [B, V, 4] clip space, tri [F, 3], one topology for all views -> rast [B, H, W, 4] = (u, v, depth z/w,
 *       triangle index + 1), zeros at an empty pixel; u, v the perspective-correct weights of corners 0 and 1.  Pixel (px, py) has its
 *       centre at NDC ((2 px + 1) / W - 1, (2 py + 1) / H - 1); no polygon clipping: a triangle with a vertex at w <= 0 or beyond the
 *       guard band is dropped whole.  cull_backfaces != 0 drops triangles of negative area.  Bit-reproducible.  F == 0 or V == 0 only
 *       zero-fills rast.  The workspace (gip_mesh_raster_workspace_size: the key buffer and the list of large triangles) is the caller's.
 *   gip_mesh_interpolate  out [B, H, W, C] = the rows idx[f][0..2] of attr [attr_batch, N, C] (attr_batch 1 or B) weighted by
 *       (u, v, 1 - u - v) of rast; idx [F, 3], or NULL for face-varying attributes (N == 3 F, row 3 f + corner).  Zeros at empty pixels.
 *   gip_mesh_interpolate_backward  g_attr [attr_batch, N, C] from g_out [B, H, W, C]; zero-filled here, then float atomic adds.
 *   gip_mesh_texture  out [B, H, W, C] = the bilinear lookup of tex [tex_batch, Th, Tw, C] (tex_batch 1 or B) at uv [B, H, W, 2]; uv
 *       (0, 0) is the corner of tex[0, 0], texel centres at (i + 0.5) / T, indices clamped at the border.
 *   gip_mesh_texture_backward  g_tex (zero-filled here, then float atomic adds; or NULL) and g_uv [B, H, W, 2] (or NULL).
 *   gip_mesh_shade  the fused forward: shaded [B, H, W, 4] = (r, g, b, alpha) with the colour the lookup of tex [Th, Tw, 3] at the
 *       interpolated face-varying uv [F, 3, 2] and alpha 1 at a covered pixel, (bg[0..2], 0) at an empty one.  flip_v != 0: uv is in the
 *       OBJ convention and every corner's v is replaced by 1 - v before it is interpolated (g_uv is then the gradient to the OBJ uv).
 *   gip_mesh_shade_backward  g_tex [Th, Tw, 3] and g_uv [F, 3, 2] (either may be NULL) from g_shaded [B, H, W, 4] (its alpha is
 *       ignored: coverage has no gradient); zero-filled here, then float atomic adds, so not bit-reproducible.
 * None of these sends a gradient to pos (the next block does).  Status 1: a NULL required pointer, B, H, W < 1, H or W > 16384, B H W > 2^31 - 1, F > 2^24 - 1 (the index
 * is stored in a float), B F > 2^31 - 1, a batch that is neither 1 nor B, a texture above 16384 a side, a short workspace.
 * Status 3: a launch error. */
int gip_mesh_raster_workspace_size(int32_t B, int32_t H, int32_t W, int64_t F, size_t* bytes);
int gip_mesh_rasterize(const float* pos, const int32_t* tri, int32_t B, int64_t V, int64_t F, int32_t H, int32_t W,
                       int32_t cull_backfaces, void* workspace, size_t workspace_bytes, float* rast, void* stream);
int gip_mesh_interpolate(const float* attr, int32_t attr_batch, int64_t N, int32_t C, const int32_t* idx, int64_t F, const float* rast,
                         int32_t B, int32_t H, int32_t W, float* out, void* stream);
int gip_mesh_interpolate_backward(const float* g_out, int32_t attr_batch, int64_t N, int32_t C, const int32_t* idx, int64_t F,
                                  const float* rast, int32_t B, int32_t H, int32_t W, float* g_attr, void* stream);
int gip_mesh_texture(const float* tex, int32_t tex_batch, int32_t Th, int32_t Tw, int32_t C, const float* uv, int32_t B, int32_t H,
                     int32_t W, float* out, void* stream);
int gip_mesh_texture_backward(const float* tex, int32_t tex_batch, int32_t Th, int32_t Tw, int32_t C, const float* uv, const float* g_out,
                              int32_t B, int32_t H, int32_t W, float* g_tex, float* g_uv, void* stream);
int gip_mesh_shade(const float* rast, const float* uv, int64_t F, int32_t flip_v, const float* tex, int32_t Th, int32_t Tw, const float* bg, int32_t B,
                   int32_t H, int32_t W, float* shaded, void* stream);
int gip_mesh_shade_backward(const float* rast, const float* uv, int64_t F, int32_t flip_v, const float* tex, int32_t Th, int32_t Tw, const float* g_shaded,
                            int32_t B, int32_t H, int32_t W, float* g_tex, float* g_uv, void* stream);
/* Gradients to vertex positions and the antialias pass (csrc/mesh_grad.hip, whose header states the definitions; the opt-in
 * DiffMeshRasterizerContext and render_mesh(position_gradients=, antialias=) of gaussianip_amd/utils/rasterize.py).
 *   gip_mesh_rasterize_backward  nvdiffrast's rasterize backward (dr.rasterize differentiated in pos, without rast_db): dL/dpos of the
 *       three corners of every covered pixel from g_rast [B, H, W, 4] (channels 0..2 = dL/d(u, v, depth); channel 3 is ignored), added
 *       with float atomic adds into g_pos [B, V, 4], WHICH THE CALLER HAS ZEROED (several calls may accumulate into one buffer).
 *   gip_mesh_interpolate_backward_rast  the rast half of dr.interpolate's backward: g_rast [B, H, W, 4] = (g_u, g_v, 0, 0) from g_out
 *       [B, H, W, C] and attr; every pixel is written (zeros at an empty one), no atomics.  idx may be NULL as in gip_mesh_interpolate.
 *   gip_mesh_shade_backward_rast  the same for the fused shade (dr.interpolate of the uv followed by dr.texture, differentiated in
 *       rast): the arguments of gip_mesh_shade_backward with g_rast [B, H, W, 4] in place of g_tex / g_uv.
 *   gip_mesh_antialias  dr.antialias: out [B, H, W, C] from color [B, H, W, C], rast, pos and tri, with topo [F, 3] the table of
 *       edge_topology (per edge: the opposite vertex of the neighbouring face, -1 without a neighbour, -2 with more than one) in place of
 *       nvdiffrast's topology hash.  A gather: bit-reproducible.
 *   gip_mesh_antialias_backward  dr.antialias's backward: g_color [B, H, W, C] (every pixel written, a gather; or NULL) and g_pos
 *       [B, V, 4] (float atomic adds into what THE CALLER HAS ZEROED; or NULL) from g_out [B, H, W, C].
 * Status as above; additionally 1 for C < 1 or B H W C > 2^31 - 1 in the antialias pair. */
int gip_mesh_rasterize_backward(const float* pos, const int32_t* tri, int32_t B, int64_t V, int64_t F, int32_t H, int32_t W, const float* rast,
                                const float* g_rast, float* g_pos, void* stream);
int gip_mesh_interpolate_backward_rast(const float* g_out, const float* attr, int32_t attr_batch, int64_t N, int32_t C, const int32_t* idx,
                                       int64_t F, const float* rast, int32_t B, int32_t H, int32_t W, float* g_rast, void* stream);
int gip_mesh_shade_backward_rast(const float* rast, const float* uv, int64_t F, int32_t flip_v, const float* tex, int32_t Th, int32_t Tw,
                                 const float* g_shaded, int32_t B, int32_t H, int32_t W, float* g_rast, void* stream);
int gip_mesh_antialias(const float* color, int32_t C, const float* rast, const float* pos, const int32_t* tri, const int32_t* topo, int32_t B,
                       int64_t V, int64_t F, int32_t H, int32_t W, float* out, void* stream);
int gip_mesh_antialias_backward(const float* color, int32_t C, const float* rast, const float* pos, const int32_t* tri, const int32_t* topo,
                                int32_t B, int64_t V, int64_t F, int32_t H, int32_t W, const float* g_out, float* g_color, float* g_pos,
                                void* stream);
/* Pixel differentials and the mipmapped lookup (csrc/mesh_mip.hip, whose header states the definitions; the opt-in
 * MipMeshRasterizerContext of gaussianip_amd/utils/rasterize.py).  The reference lines are those of threestudio/utils/rasterize.py.
 *   gip_mesh_rast_db  the second value of dr.rasterize(..., grad_db=True) (rasterize.py:37, rasterize_one's rast_db[0] at :47): rast_db
 *       [B, H, W, 4] = (du/dX, du/dY, dv/dX, dv/dY) in pixels from pos, tri and the rast of gip_mesh_rasterize; zeros at an empty
 *       pixel.  F == 0 or V == 0 only zero-fills.  No gradient to pos is defined through it (nvdiffrast's grad_db = False).
 *   gip_mesh_interpolate_da  dr.interpolate(..., rast_db=, diff_attrs=) (rasterize.py:66-68): out_da [B, H, W, 2 K] = (da/dX, da/dY) of
 *       the K channels `channels` [K] int32 lists on the device (NULL: K == C, all channels in order); a listed channel outside [0, C)
 *       reads nothing and gives zeros.  The other arguments are those of gip_mesh_interpolate.
 *   gip_mesh_interpolate_da_backward  its backward to attr: g_attr [attr_batch, N, C] from g_da [B, H, W, 2 K]; zero-filled here, then
 *       float atomic adds.  Nothing reaches rast or rast_db.
 *   gip_mesh_mip_levels  host only: *levels = L, the index of the last level of the stack of a Th x Tw texture (max_level < 0: no cap),
 *       *texels = the texels of levels 1 .. L together, which is what `mip` holds per texture (times C floats).
 *   gip_mesh_mip_build  dr.texture_construct_mip: levels 1 .. L of tex [tex_batch, Th, Tw, C] into mip [tex_batch, mip_texels, C], one
 *       launch per level; L == 0 launches nothing.  mip_texels must be what gip_mesh_mip_levels gives (status 1 otherwise).
 *   gip_mesh_mip_fold  the build's transpose: the gradient stack g_mip (levels L .. 1, edited in place) folded into g_tex, a gather
 *       per level, bit-reproducible.
 *   gip_mesh_texture_mip  dr.texture(..., uv_da=, mip_level_bias=, mip=, filter_mode='linear-mipmap-linear' or, nearest != 0,
 *       'linear-mipmap-nearest', boundary_mode='clamp'): out [B, H, W, C]; uv_da [B, H, W, 4] and bias [B, H, W] may each be NULL.
 *   gip_mesh_texture_mip_backward  g_tex [tex_batch, Th, Tw, C] and g_mip [tex_batch, mip_texels, C] (both zero-filled here, then float
 *       atomic adds; g_mip is needed with g_tex when L > 0, and gip_mesh_mip_fold then completes g_tex), g_uv [B, H, W, 2], g_uv_da
 *       [B, H, W, 4] (needs uv_da), g_bias [B, H, W] (needs bias); each may be NULL.
 * Status as above; additionally 1 for K < 1, B H W 2 K > 2^31 - 1, tex_batch Th Tw C > 2^31 - 1 or a mip_texels that does not match. */
int gip_mesh_rast_db(const float* pos, const int32_t* tri, int32_t B, int64_t V, int64_t F, int32_t H, int32_t W, const float* rast,
                     float* rast_db, void* stream);
int gip_mesh_interpolate_da(const float* attr, int32_t attr_batch, int64_t N, int32_t C, const int32_t* idx, int64_t F, const float* rast,
                            const float* rast_db, const int32_t* channels, int32_t K, int32_t B, int32_t H, int32_t W, float* out_da,
                            void* stream);
int gip_mesh_interpolate_da_backward(const float* g_da, int32_t attr_batch, int64_t N, int32_t C, const int32_t* idx, int64_t F,
                                     const float* rast, const float* rast_db, const int32_t* channels, int32_t K, int32_t B, int32_t H,
                                     int32_t W, float* g_attr, void* stream);
int gip_mesh_mip_levels(int32_t Th, int32_t Tw, int32_t max_level, int32_t* levels, int64_t* texels);
int gip_mesh_mip_build(const float* tex, int32_t tex_batch, int32_t Th, int32_t Tw, int32_t C, int32_t max_level, float* mip,
                       int64_t mip_texels, void* stream);
int gip_mesh_mip_fold(float* g_tex, int32_t tex_batch, int32_t Th, int32_t Tw, int32_t C, int32_t max_level, float* g_mip,
                      int64_t mip_texels, void* stream);
int gip_mesh_texture_mip(const float* tex, int32_t tex_batch, int32_t Th, int32_t Tw, int32_t C, const float* mip, int64_t mip_texels,
                         int32_t max_level, const float* uv, const float* uv_da, const float* bias, int32_t nearest, int32_t B, int32_t H,
                         int32_t W, float* out, void* stream);
int gip_mesh_texture_mip_backward(const float* tex, int32_t tex_batch, int32_t Th, int32_t Tw, int32_t C, const float* mip,
                                  int64_t mip_texels, int32_t max_level, const float* uv, const float* uv_da, const float* bias,
                                  int32_t nearest, const float* g_out, int32_t B, int32_t H, int32_t W, float* g_tex, float* g_mip,
                                  float* g_uv, float* g_uv_da, float* g_bias, void* stream);
/* Cleaning and decimating the extracted mesh (csrc/mesh_clean.hip, whose header states the definitions; gaussianip_amd/utils/mesh.py
 * connected_components, clean_mesh, cluster_decimate, decimate_mesh).  In place of the reference's third-party clean_mesh and
 * decimate_mesh (gs_renderer.py:346-350).  vertices [V, 3] float32, faces [F, 3] int32, everything on the device; a face with an index
 * outside [0, V) is skipped by every kernel.  No kernel waits on another workgroup; the loop over rounds is the caller's.
 *   gip_mesh_components_rounds  `rounds` (1 .. 64) rounds of hook + compress on labels [V] int32, WHICH THE CALLER HAS SET TO 0 .. V - 1
 *       before the first call; *changed (device int32, zeroed by the caller) is raised when a label moved.  At the fixed point
 *       labels[v] is the smallest vertex index of v's component (two vertices are connected when a face names both).
 *   gip_mesh_component_stats  per label l: face_count [V] int32 = the faces of component l, box [V, 6] float32 = (min x, y, z, max x, y,
 *       z) over the corners of its faces; integer atomics on order-preserving keys, so order-independent.  Rows of labels without a
 *       face: count 0, box undefined.  Both are initialised here.
 *   gip_mesh_cluster_keys  keys [V] int64 = (iz n + iy) n + ix with i = min((int) floorf((p - lo) / h), n - 1) per axis in float32.
 *   gip_mesh_cluster_count  *count (device int32, zeroed here) = the faces whose three corners have three different keys.
 *   gip_mesh_cluster_place  out [C, 3]: the quadric-optimal vertex of each of the C occupied cells (cell_key [C] int64 ascending),
 *       clamped to its cell.  corner_order [3 F] int32: the face corners 3 f + k stably sorted by the cell of their vertex, corner_start
 *       [C + 1] int32 the cells' offsets into it; member_order [V] int32 / member_start [C + 1] the same for the vertices.  `lanes` (16,
 *       32 or 64) lanes walk a cell's runs in order and add their partial sums in a fixed tree: a gather, no float atomics, bitwise
 *       equal from run to run (the last bits depend on `lanes`).
 * Status 1: a NULL required pointer, V > 2^31 - 1, 3 F > 2^31 - 1, n outside 1 .. 2048, h not a positive finite number, C > V, lanes
 * not 16, 32 or 64, rounds outside 1 .. 64; a call that fails so launches nothing.  Status 3: a launch error. */
int gip_mesh_components_rounds(const int32_t* faces, int64_t F, int64_t V, int32_t* labels, int32_t* changed, int32_t rounds, void* stream);
int gip_mesh_component_stats(const float* vertices, const int32_t* faces, int64_t F, int64_t V, const int32_t* labels, int32_t* face_count,
                             float* box, void* stream);
int gip_mesh_cluster_keys(const float* vertices, int64_t V, float lo_x, float lo_y, float lo_z, float h, int32_t n, int64_t* keys, void* stream);
int gip_mesh_cluster_count(const float* vertices, int64_t V, const int32_t* faces, int64_t F, float lo_x, float lo_y, float lo_z, float h,
                           int32_t n, int32_t* count, void* stream);
int gip_mesh_cluster_place(const float* vertices, int64_t V, const int32_t* faces, int64_t F, const int64_t* cell_key, int64_t C,
                           const int32_t* corner_order, const int32_t* corner_start, const int32_t* member_order, const int32_t* member_start,
                           float lo_x, float lo_y, float lo_z, float h, int32_t n, int32_t lanes, float* out, void* stream);
/* Geometry terms of a mesh-fitting loop (csrc/mesh_geom.hip, whose header states the definitions; gaussianip_amd/utils/mesh_geometry.py
 * MeshTopology, vertex_normals, laplacian_loss, normal_consistency): the reference's Mesh.v_nrm, Mesh.laplacian() and
 * Mesh.normal_consistency() (threestudio/models/mesh.py) with their backward passes.  pos [V, 3] float32 of one mesh, faces [F, 3] int32,
 * and the tables built once per face list: corner_start [V + 1] / corner_list [3 F] (the corners 3 f + k grouped by vertex, ascending),
 * nbr_start [V + 1] / nbr_list [N] (per vertex its distinct neighbours, ascending), E the number of unique undirected edges (pairs
 * (a, a) included).  Every kernel is a gather, one lane per vertex: no float atomics, forward and backward bitwise equal from run to run.
 *   gip_mesh_geometry_workspace_size  *bytes = the partial sums of the two losses (one float per workgroup of 256 vertices).
 *   gip_mesh_vertex_normals  n [V, 3] and len [V] (|s_v|, 0 where the default normal (0, 0, 1) was taken).  face_normals [F, 3] is the
 *       caller's buffer for the per-face cross products, which a first pass fills and the gather reads.
 *   gip_mesh_vertex_normals_backward  g_pos [V, 3] from g_n [V, 3]; g_s [V, 3] is the caller's buffer for the gradient behind the
 *       normalisation.
 *   gip_mesh_laplacian_loss  *loss (device) = mean_v |sum_j (p_v - p_j)|; unit [V, 3] = that vector normalised (0 where it is 0), kept
 *       for gip_mesh_laplacian_loss_backward, which reads the upstream gradient from the device scalar g_loss.
 *   gip_mesh_normal_consistency  *loss (device) = (1 / E) sum over the edges of 1 - cos(n_a, n_b); gip_mesh_normal_consistency_backward
 *       gives g_n [V, 3].
 * Status 1: a NULL required pointer, V, 3 F or N outside 0 .. 2^31 - 1, E < 0, a short workspace; a call that fails so launches nothing.
 * V == 0 (and F == 0 for the normals, E == 0 for the consistency) is a success that launches nothing and writes nothing.  Status 3: a
 * launch error. */
int gip_mesh_geometry_workspace_size(int64_t V, size_t* bytes);
int gip_mesh_vertex_normals(const float* pos, const int32_t* faces, const int32_t* corner_start, const int32_t* corner_list, int64_t V,
                            int64_t F, float* face_normals, float* n, float* len, void* stream);
int gip_mesh_vertex_normals_backward(const float* pos, const int32_t* faces, const int32_t* corner_start, const int32_t* corner_list,
                                     const float* n, const float* len, const float* g_n, int64_t V, int64_t F, float* g_s, float* g_pos,
                                     void* stream);
int gip_mesh_laplacian_loss(const float* pos, const int32_t* nbr_start, const int32_t* nbr_list, int64_t V, int64_t N, float* unit,
                            float* loss, void* workspace, size_t workspace_bytes, void* stream);
int gip_mesh_laplacian_loss_backward(const float* unit, const int32_t* nbr_start, const int32_t* nbr_list, const float* g_loss, int64_t V,
                                     int64_t N, float* g_pos, void* stream);
int gip_mesh_normal_consistency(const float* n, const int32_t* nbr_start, const int32_t* nbr_list, int64_t V, int64_t N, int64_t E,
                                float* loss, void* workspace, size_t workspace_bytes, void* stream);
int gip_mesh_normal_consistency_backward(const float* n, const int32_t* nbr_start, const int32_t* nbr_list, const float* g_loss, int64_t V,
                                         int64_t N, int64_t E, float* g_n, void* stream);
/* Unwrapping the mesh into a chart atlas, tangents and seam padding (csrc/mesh_uv.hip, whose header states the definitions and the
 * float32 arithmetic; gaussianip_amd/utils/uv_atlas.py unwrap_charts, vertex_tangents, dilate_texture).  pos [V, 3] float32, faces
 * [F, 3] int32, face_nbr [F, 3] int32 (the face across edge (k, k + 1 mod 3) or -1: uv_atlas.face_adjacency), everything on the device.
 *   gip_uv_face_classes  with gip_uv_chart_rounds, gip_uv_chart_boxes and gip_uv_place in place of xatlas' chart and pack passes
 *       (threestudio/models/mesh.py:207-250, Mesh._unwrap_uv).  normals [F, 3] = cross(p1 - p0, p2 - p0); smooth_rounds (0 .. 64)
 *       gather rounds over face_nbr ping-pong between smooth_a and smooth_b [F, 3] (unused and may be NULL at 0 rounds); face_class [F]
 *       = 2 axis + sign of the smoothed normal where the face keeps min_cos (0 .. 0.5) of its area in that projection, else of its own
 *       normal; 4 for a face with |n|^2 <= 1e-20.
 *   gip_uv_chart_rounds  `rounds` (1 .. 64) rounds of hook + compress on labels [F] int32, WHICH THE CALLER HAS SET TO 0 .. F - 1 before
 *       the first call, over the face_nbr entries that join two faces of one class; *changed (device int32, zeroed by the caller) is
 *       raised when a label moved.  At the fixed point labels[f] is the smallest face index of f's chart.
 *   gip_uv_chart_boxes  box_keys [C, 4] uint32 = (min u, min v, max u, max v) of every chart's corners in the projection of
 *       chart_class [C], as order-preserving keys (a non-negative float's bits | 0x80000000, a negative one's bits inverted); THE
 *       CALLER INITIALISES the minima to 0xffffffff and the maxima to 0 and decodes.  Integer atomics only: order-independent.
 *   gip_uv_place  v_tex [Vt, 2]: texture vertex t is position vertex vmapping[t] in chart vt_chart[t], placed with the chart's row of
 *       chart_origin [C, 4] = (umin, vmin, x0 + pad, y0 + pad) and `scale` texels per unit, as OBJ coordinates of a texture_size^2 image.
 *   gip_uv_vertex_tangents  the reference's Mesh._compute_vertex_tangent (mesh.py:162-205) as a gather over corner_start [V + 1] /
 *       corner_list [3 F] (MeshTopology): tangents [V, 3] from pos, nrm [V, 3], v_tex [Vt, 2] and tex_idx [F, 3]; face_tangents [F, 3]
 *       is the caller's buffer, kept for the backward.  A vertex without a corner gets (1, 0, 0).
 *   gip_uv_vertex_tangents_backward  g_pos [V, 3] and g_nrm [V, 3] from g_tangents [V, 3] (autograd through mesh.py:162-205 with v_tex
 *       constant); g_sum [V, 3] and g_edge [F, 6] are the caller's buffers.  No float atomics in either direction.
 *   gip_texture_dilate  in place of cv2.inpaint (mesh_exporter.py:113-121): `rounds` rounds that give an unfilled texel with a filled
 *       8-neighbour their mean; tex_a [H, W, C] / mask_a [H, W] uint8 hold the input, round r writes the other pair, so the result is
 *       in (tex_a, mask_a) when rounds is even and in (tex_b, mask_b) when it is odd.
 * Status 1: a NULL required pointer, V or 3 F above 2^31 - 1, smooth_rounds, min_cos, rounds, C or texture_size out of range, scale not
 * positive, H or W outside 1 .. 16384, channels outside 1 .. 64; a call that fails so launches nothing.  Empty input (F == 0, Vt == 0,
 * V == 0, rounds == 0 of the dilation) is a success that launches nothing.  Status 3: a launch error. */
int gip_uv_face_classes(const float* pos, const int32_t* faces, const int32_t* face_nbr, int64_t V, int64_t F, int32_t smooth_rounds,
                        float min_cos, float* normals, float* smooth_a, float* smooth_b, int32_t* face_class, void* stream);
int gip_uv_chart_rounds(const int32_t* face_nbr, const int32_t* face_class, int64_t F, int32_t* labels, int32_t* changed, int32_t rounds,
                        void* stream);
int gip_uv_chart_boxes(const float* pos, const int32_t* faces, const int32_t* face_chart, const int32_t* chart_class, int64_t V, int64_t F,
                       int64_t C, uint32_t* box_keys, void* stream);
int gip_uv_place(const float* pos, const int32_t* vmapping, const int32_t* vt_chart, const int32_t* chart_class, const float* chart_origin,
                 int64_t V, int64_t Vt, int64_t C, float scale, int32_t texture_size, float* v_tex, void* stream);
int gip_uv_vertex_tangents(const float* pos, const int32_t* faces, const int32_t* corner_start, const int32_t* corner_list,
                           const int32_t* tex_idx, const float* v_tex, const float* nrm, int64_t V, int64_t F, int64_t Vt,
                           float* face_tangents, float* tangents, void* stream);
int gip_uv_vertex_tangents_backward(const int32_t* faces, const int32_t* corner_start, const int32_t* corner_list, const int32_t* tex_idx,
                                    const float* v_tex, const float* nrm, const float* face_tangents, const float* g_tangents, int64_t V,
                                    int64_t F, int64_t Vt, float* g_sum, float* g_edge, float* g_pos, float* g_nrm, void* stream);
int gip_texture_dilate(float* tex_a, uint8_t* mask_a, float* tex_b, uint8_t* mask_b, int32_t H, int32_t W, int32_t C, int32_t rounds,
                       void* stream);
/* Differentiable marching tetrahedra over a tetrahedral grid and the tet_sdf_diff regulariser (csrc/mesh_tets.hip, whose header states
 * the definitions; gaussianip_amd/utils/isosurface.py TetGrid, marching_tetrahedra, tet_sdf_diff).  sdf [Nv] and pos [Nv, 3] float32;
 * the grid's tables, built once: edges [Ne, 2] (a < b, lexicographic), tets [Ft, 4], tet_edge_ids [Ft, 6], vert_edge_start [Nv + 1] and
 * vert_edge_list [2 Ne] (entries 2 e + end, ascending per vertex), all int32; everything on the device.
 *   gip_tet_mark  flags [Ne + 2 Ft] int32: per edge whether it crosses, per tetrahedron whether it emits one triangle, and whether two.
 *   gip_tet_emit  with `scan`, the caller's inclusive int32 scan of all of `flags`, and the three totals read from it (V vertices, F1
 *       one-triangle and F2 two-triangle tetrahedra): v_pos [V, 3], faces [F1 + 2 F2, 3] int32 and edge_vid [Ne] int32 (-1: no crossing).
 *   gip_tet_backward  g_sdf [Nv] and, unless g_pos is NULL, g_pos [Nv, 3] from g_v [V, 3]: a gather per grid vertex, no atomics.
 *   gip_tet_sdf_diff  *loss (device) and *count (device, the number of edges whose ends differ in sign; loss 0 when it is 0);
 *       workspace of gip_tet_workspace_size(Ne) bytes.  gip_tet_sdf_diff_backward reads count and the upstream gradient g_loss from the
 *       device and writes g_sdf [Nv].
 * Status 1: a NULL required pointer, Nv above 2^31 - 1, 2 Ne, 6 Ft or Ne + 2 Ft above 2^31 - 1, totals that do not fit the grid, a short
 * workspace; a call that fails so launches nothing.  Nothing to do (no edge, no grid vertex) is a success that launches nothing.
 * Status 3: a launch error. */
int gip_tet_workspace_size(int64_t Ne, size_t* bytes);
int gip_tet_mark(const float* sdf, const int32_t* edges, const int32_t* tets, int64_t Nv, int64_t Ne, int64_t Ft, int32_t* flags, void* stream);
int gip_tet_emit(const float* pos, const float* sdf, const int32_t* edges, const int32_t* tets, const int32_t* tet_edge_ids,
                 const int32_t* flags, const int32_t* scan, int64_t Nv, int64_t Ne, int64_t Ft, int64_t V, int64_t F1, int64_t F2, float* v_pos,
                 int32_t* faces, int32_t* edge_vid, void* stream);
int gip_tet_backward(const float* pos, const float* sdf, const int32_t* edges, const int32_t* vert_edge_start, const int32_t* vert_edge_list,
                     const int32_t* edge_vid, const float* g_v, int64_t Nv, int64_t Ne, int64_t V, float* g_pos, float* g_sdf, void* stream);
int gip_tet_sdf_diff(const float* sdf, const int32_t* edges, int64_t Nv, int64_t Ne, float* loss, int32_t* count, void* workspace,
                     size_t workspace_bytes, void* stream);
int gip_tet_sdf_diff_backward(const float* sdf, const int32_t* edges, const int32_t* vert_edge_start, const int32_t* vert_edge_list,
                              const int32_t* count, const float* g_loss, int64_t Nv, int64_t Ne, float* g_sdf, void* stream);
/* A multiresolution hash-grid encoding of 3-D points, forward and both backward passes (csrc/hashgrid.hip, whose header states the
 * definition; gaussianip_amd/utils/encoding.py HashGridLayout, hash_grid_encode).  x [N, 3], table [P, F], enc and g_enc [N, L F]
 * (level-major), g_x [N, 3], g_table [P, F]: float32 on the device; table, enc and g_enc aligned to min(4 F, 16) bytes.  The level table
 * is five HOST arrays of L entries: level_scale (float32), level_res, level_size (rows of the level's slice, 1 .. 2^24), level_offset
 * (int64, the running sum of the sizes, which must total P) and level_hashed (0: dense rows, else hashed rows).
 *   gip_hashgrid_forward         enc; no atomics, bitwise reproducible.
 *   gip_hashgrid_backward_input  g_x, a gather over the same walk; no atomics, bitwise reproducible.
 *   gip_hashgrid_backward_table  ADDS into g_table, which the caller zeroed, with float atomic adds: the one output that is not bitwise
 *       reproducible from run to run.
 * Status 1: a NULL required pointer, L outside 1 .. 32, F not 1, 2, 4 or 8, N < 0, 4 N L F above 2^32 - 1, a level whose scale is not
 * finite, whose res is below 1 or whose size is outside 1 .. 2^24, offsets that are not the running sum, sizes that do not total P, a
 * misaligned table, enc or g_enc; a call that fails so launches nothing.  N == 0 is a success that launches nothing (the level table is
 * still checked).  Status 3: a launch error. */
int gip_hashgrid_forward(const float* x, const float* table, const float* level_scale, const int32_t* level_res, const int32_t* level_size,
                         const int64_t* level_offset, const int32_t* level_hashed, int64_t N, int32_t L, int32_t F, int64_t P, float* enc,
                         void* stream);
int gip_hashgrid_backward_input(const float* x, const float* table, const float* g_enc, const float* level_scale, const int32_t* level_res,
                                const int32_t* level_size, const int64_t* level_offset, const int32_t* level_hashed, int64_t N, int32_t L,
                                int32_t F, int64_t P, float* g_x, void* stream);
int gip_hashgrid_backward_table(const float* x, const float* g_enc, const float* level_scale, const int32_t* level_res,
                                const int32_t* level_size, const int64_t* level_offset, const int32_t* level_hashed, int64_t N, int32_t L,
                                int32_t F, int64_t P, float* g_table, void* stream);
/* Volume rendering of a density field: marching rays through an occupancy grid and compositing along them (csrc/volume.hip, whose
 * header states the definition; gaussianip_amd/utils/volume.py).  They stand in for the nerfacc calls of the reference's
 * nerf-volume-renderer (threestudio/models/renderers/nerf_volume_renderer.py); nerfacc is CUDA-only.  All arrays are on the device:
 * rays_o, rays_d [R, 3] float32, occ [G, G, G] uint8 ([ix, iy, iz]), jitter [R] float32 or NULL, counts [R] int32, offsets [R + 1]
 * int32 (CSR: the samples of ray r are the rows offsets[r] .. offsets[r + 1] - 1), ray_indices [M] int32, every other array float32.
 * The box lo, hi and scale = G / (hi - lo) per axis go by value.  No entry point uses an atomic: every output is bitwise reproducible.
 *   gip_volume_march_count, gip_volume_march_emit   nerfacc.OccGridEstimator.sampling without its sigma_fn (nerf_volume_renderer.py:84
 *       and :96): the number of samples of every ray; then, with offsets = the exclusive running sum of the counts and M their total,
 *       ray_indices, t_starts and t_ends [M], a ray's samples adjacent and ordered by t.  A row is compared with M before it is written.
 *   gip_volume_weights_forward / _backward          nerfacc.render_weight_from_density (nerf_volume_renderer.py:150): weights, trans and
 *       alphas [M] of sigmas [M]; backward g_sigmas [M] of g_weights [M] and the forward's three outputs.  Rows are clamped to [0, M].
 *   gip_volume_accumulate_forward / _backward       nerfacc.accumulate_along_rays (nerf_volume_renderer.py:158, :161, :164, :170):
 *       out [R, C] = the weighted sum of values [M, C] along each ray, C = 1 .. 16; values NULL means ones and C = 1.  Backward writes
 *       g_weights [M] and g_values [M, C] (either may be NULL) of g_out [R, C]; a ray index outside [0, R) gives zeros.
 * Status 1, launching nothing: a NULL required pointer, R < 0 or R above (2^31 - 1) / 64, G outside 1 .. 256, K_cap < 1,
 * R K_cap >= 2^31, dt not positive and finite, a NaN near or far, a box that is not finite with lo < hi and scale > 0, M outside
 * 0 .. 2^31 - 1, C outside 1 .. 16, C != 1 without values, M C >= 2^31.  R == 0 (and, where nothing would be written, M == 0) is a
 * success that launches nothing.  Status 3: a launch error. */
int gip_volume_march_count(const float* rays_o, const float* rays_d, const uint8_t* occ, const float* jitter, int64_t R, int32_t G,
                           float lo_x, float lo_y, float lo_z, float hi_x, float hi_y, float hi_z, float scale_x, float scale_y,
                           float scale_z, float dt, float near, float far, int32_t K_cap, int32_t* counts, void* stream);
int gip_volume_march_emit(const float* rays_o, const float* rays_d, const uint8_t* occ, const float* jitter, int64_t R, int32_t G,
                          float lo_x, float lo_y, float lo_z, float hi_x, float hi_y, float hi_z, float scale_x, float scale_y,
                          float scale_z, float dt, float near, float far, int32_t K_cap, const int32_t* offsets, int64_t M,
                          int32_t* ray_indices, float* t_starts, float* t_ends, void* stream);
int gip_volume_weights_forward(const float* t_starts, const float* t_ends, const float* sigmas, const int32_t* offsets, int64_t R, int64_t M,
                               float* weights, float* trans, float* alphas, void* stream);
int gip_volume_weights_backward(const float* t_starts, const float* t_ends, const float* g_weights, const float* weights, const float* trans,
                                const float* alphas, const int32_t* offsets, int64_t R, int64_t M, float* g_sigmas, void* stream);
int gip_volume_accumulate_forward(const float* weights, const float* values, const int32_t* offsets, int64_t R, int64_t M, int32_t C,
                                  float* out, void* stream);
int gip_volume_accumulate_backward(const float* weights, const float* values, const int32_t* ray_indices, const float* g_out, int64_t R,
                                   int64_t M, int32_t C, float* g_weights, float* g_values, void* stream);
/* NeuS volume rendering of a signed-distance field (csrc/volume_sdf.hip, whose header states the definition;
 * gaussianip_amd/utils/sdf_volume.py).  They stand in for what the reference's neus-volume-renderer
 * (threestudio/models/renderers/neus_volume_renderer.py) computes with PyTorch ops and nerfacc.  All arrays are on the device and
 * float32 but offsets [R + 1] int32 (CSR, as above): sdf, t_starts, t_ends, alphas, trans, weights [M], normals [M, 3] or NULL (then
 * iter_cos = -1, the alpha_fn form), rays_d [R, 3] (indexed by the ray), values [M, C] or NULL (then C = 0), inv_std one float read on
 * the device, cos_anneal_ratio by value, out and g_out [R, 2 + C] (opacity, depth, the C channels).  No entry point uses an atomic:
 * every output is bitwise reproducible.
 *   gip_volume_alpha_weights_forward / _backward    nerfacc.render_weight_from_alpha (neus_volume_renderer.py:216): weights and trans [M]
 *       of alphas [M]; backward g_alphas [M] of g_weights [M] by the division-free reverse recurrence, finite at alpha == 1.
 *   gip_volume_sdf_render_forward                   get_alpha with use_volsdf off (:72-96; normals NULL: alpha_fn :135-141 and occ_eval_fn
 *       :295-301), render_weight_from_alpha (:216) and the accumulate_along_rays calls (:222, :225, :228, :262) in one launch: alphas,
 *       trans, weights [M] and out [R, 2 + C].
 *   gip_volume_sdf_render_backward                  their backward in one launch: g_sdf [M], g_normals [M, 3] (NULL allowed; needs normals),
 *       g_values [M, C] (NULL allowed) and g_inv_std_rays [R], the per-ray parts of inv_std's gradient, which the caller adds; of g_out
 *       [R, 2 + C] and g_weights [M] (NULL allowed).  No gradient to the rays or the samples.
 * Status 1, launching nothing: a NULL required pointer, R < 0 or R above (2^31 - 1) / 64, M outside 0 .. 2^31 - 1, C outside 0 .. 16,
 * values NULL with C != 0 or given with C == 0, M max(C, 1) >= 2^31, cos_anneal_ratio not finite or outside [0, 1].  R == 0 or M == 0
 * is a success that launches nothing.  Status 3: a launch error. */
int gip_volume_alpha_weights_forward(const float* alphas, const int32_t* offsets, int64_t R, int64_t M, float* weights, float* trans,
                                     void* stream);
int gip_volume_alpha_weights_backward(const float* alphas, const float* trans, const float* g_weights, const int32_t* offsets, int64_t R,
                                      int64_t M, float* g_alphas, void* stream);
int gip_volume_sdf_render_forward(const float* sdf, const float* normals, const float* rays_d, const float* t_starts, const float* t_ends,
                                  const float* values, const int32_t* offsets, const float* inv_std, float cos_anneal_ratio, int64_t R,
                                  int64_t M, int32_t C, float* alphas, float* trans, float* weights, float* out, void* stream);
int gip_volume_sdf_render_backward(const float* sdf, const float* normals, const float* rays_d, const float* t_starts, const float* t_ends,
                                   const float* values, const int32_t* offsets, const float* inv_std, float cos_anneal_ratio,
                                   const float* alphas, const float* trans, const float* weights, const float* g_out, const float* g_weights,
                                   int64_t R, int64_t M, int32_t C, float* g_sdf, float* g_normals, float* g_values, float* g_inv_std_rays,
                                   void* stream);
#ifdef __cplusplus
}
#endif
#endif
