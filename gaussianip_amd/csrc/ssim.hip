// ssim.hip — the structural-similarity loss of the 3DGS trainers (gaussiansplatting/utils/loss_utils.py:33-63 ssim / _ssim) as
// ONE forward and ONE backward kernel (+ a one-workgroup-per-image finishing pass of the reduction), linked into libgip_model.so.
//
// Definition (the reference's, depthwise per (n, c) plane of [N, C, H, W] float32): with blur() the 11 x 11 Gaussian window
// (sigma 1.5, normalised in float32) applied with ZERO padding of 5 pixels,
//   mu1 = blur(x), mu2 = blur(y), s1 = blur(x^2) - mu1^2, s2 = blur(y^2) - mu2^2, s12 = blur(x y) - mu1 mu2,
//   A1 = 2 mu1 mu2 + C1, A2 = 2 s12 + C2, B1 = mu1^2 + mu2^2 + C1, B2 = s1 + s2 + C2, m = A1 A2 / (B1 B2),  C1 = 0.01^2, C2 = 0.03^2.
// The reference spells it as five grouped 121-tap F.conv2d calls and a dozen pointwise ops; here the window is applied separably
// (11 + 11 taps) inside one workgroup per 32 x 32 output tile:
//   stage   both images' 42 x 42 tile-plus-halo into LDS, zeros outside the image (that IS the padding: no per-tap branch),
//   rows    11-tap horizontal pass -> five row-filtered planes [42][32] in LDS  (x, y, x^2, y^2, x y),
//   columns 11-tap vertical pass from LDS into registers: a thread owns 4 vertically adjacent pixels of one column and slides
//           over 14 rows per plane,
//   m, its three derivative planes (when asked for), the tile's sum of m -> one partial per workgroup.
// LDS: 2 * 42 * 42 * 4 + 5 * 42 * 32 * 4 = 40,992 bytes forward (3 workgroups of 4 waves per CU), 3 * (42 * 42 + 42 * 32) * 4 =
// 37,296 bytes backward (4 per CU).
//
// What the forward keeps for the backward (3 planes instead of the 5 moment maps autograd keeps):
//   r1 = A1 / B1, r2 = A2 / B2, m = r1 r2
//   d_s1 = dm/ds1 = -m / B2,     d_s12 = dm/ds12 = 2 r1 / B2,
//   d_mu = dm/dmu1 - 2 mu1 d_s1 - mu2 d_s12 = 2 (mu2 r2 - mu1 m) / B1 + 2 (mu1 m - mu2 r1) / B2
//   dL/dx = s (blur(d_mu) + 2 x blur(d_s1) + y blur(d_s12))          (the blur is symmetric and zero padded: its own adjoint)
// In this spelling img2 == img1 gives r1 = r2 = m = 1 exactly, d_mu = 0 and d_s12 = -2 d_s1 bit for bit, so the gradient at the
// maximum of the SSIM is exactly zero instead of the rounding residue of three large cancelling terms.
//
// Built with -ffp-contract=off: the only fused multiply-adds are the explicit fmaf() of the window taps (one rounding per tap,
// the same instruction whatever the compiler version).  No float atomics: per-workgroup partial sums go to the caller's workspace
// and ssim_finish_kernel adds them in one fixed order (double accumulators) -> two runs are bitwise equal.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gip_model.h"

#define SSIM_TILE 32
#define SSIM_HALO 5
#define SSIM_EXT (SSIM_TILE + 2 * SSIM_HALO)   // 42
#define SSIM_THREADS 256
#define SSIM_ROWS_PER_THREAD (SSIM_TILE * SSIM_TILE / SSIM_THREADS)   // 4

// exp(-(i - 5)^2 / 4.5) evaluated in double, rounded to float32, divided by their float32 sum (3.75923276): the float32 values of
// loss_utils.py:23-25 gaussian(11, 1.5), written as exact hexadecimal literals
#define SSIM_W0 0x1.0d956cp-10f
#define SSIM_W1 0x1.f1fe02p-8f
#define SSIM_W2 0x1.26eb18p-5f
#define SSIM_W3 0x1.bff0fep-4f
#define SSIM_W4 0x1.b43c3ep-3f
#define SSIM_W5 0x1.10656p-2f

// 11 taps on values held in registers (v[0 .. 10]), one fixed order
#define SSIM_TAPS(v, o)                                                                                                          \
  fmaf(SSIM_W0, (v)[(o) + 10],                                                                                                   \
       fmaf(SSIM_W1, (v)[(o) + 9],                                                                                               \
            fmaf(SSIM_W2, (v)[(o) + 8],                                                                                          \
                 fmaf(SSIM_W3, (v)[(o) + 7],                                                                                     \
                      fmaf(SSIM_W4, (v)[(o) + 6],                                                                                \
                           fmaf(SSIM_W5, (v)[(o) + 5],                                                                           \
                                fmaf(SSIM_W4, (v)[(o) + 4],                                                                      \
                                     fmaf(SSIM_W3, (v)[(o) + 3],                                                                 \
                                          fmaf(SSIM_W2, (v)[(o) + 2], fmaf(SSIM_W1, (v)[(o) + 1], SSIM_W0 * (v)[(o)]))))))))))

struct SsimTile {
  int64_t plane;   // n * C + c
  int y0, x0;      // top-left output pixel of the tile
};

__device__ __forceinline__ SsimTile ssim_tile(int tiles_x, int tiles_y) {
  const int64_t b = blockIdx.x;
  const int per_plane = tiles_x * tiles_y;
  SsimTile t;
  t.plane = b / per_plane;
  const int r = (int)(b - t.plane * per_plane);
  t.y0 = (r / tiles_x) * SSIM_TILE;
  t.x0 = (r % tiles_x) * SSIM_TILE;
  return t;
}

// the tile plus its halo of one plane into LDS; zero outside the image
__device__ __forceinline__ void ssim_stage(const float* __restrict__ src, int H, int W, int y0, int x0, float (*dst)[SSIM_EXT]) {
  for (int i = threadIdx.x; i < SSIM_EXT * SSIM_EXT; i += SSIM_THREADS) {
    const int r = i / SSIM_EXT, c = i - r * SSIM_EXT;
    const int gy = y0 - SSIM_HALO + r, gx = x0 - SSIM_HALO + c;
    dst[r][c] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? src[(int64_t)gy * W + gx] : 0.f;
  }
}

// the vertical pass of one row-filtered plane for the 4 pixels (rows ty*4 .. ty*4+3, column tx) of this thread
__device__ __forceinline__ void ssim_columns(const float (*h)[SSIM_TILE], int ty, int tx, float out[SSIM_ROWS_PER_THREAD]) {
  float v[SSIM_ROWS_PER_THREAD + 2 * SSIM_HALO];
#pragma unroll
  for (int k = 0; k < SSIM_ROWS_PER_THREAD + 2 * SSIM_HALO; k++) v[k] = h[ty * SSIM_ROWS_PER_THREAD + k][tx];
#pragma unroll
  for (int j = 0; j < SSIM_ROWS_PER_THREAD; j++) out[j] = SSIM_TAPS(v, j);
}

__global__ void __launch_bounds__(SSIM_THREADS)
ssim_forward_kernel(const float* __restrict__ img1, const float* __restrict__ img2, int H, int W, int tiles_x, int tiles_y,
                    float* __restrict__ deriv, int64_t plane_stride_all, float* __restrict__ map, float* __restrict__ partial) {
  __shared__ float s_x[SSIM_EXT][SSIM_EXT], s_y[SSIM_EXT][SSIM_EXT];
  __shared__ float s_h[5][SSIM_EXT][SSIM_TILE];
  __shared__ float s_red[SSIM_THREADS / 64];
  const SsimTile t = ssim_tile(tiles_x, tiles_y);
  const int64_t base = t.plane * H * W;
  ssim_stage(img1 + base, H, W, t.y0, t.x0, s_x);
  ssim_stage(img2 + base, H, W, t.y0, t.x0, s_y);
  __syncthreads();
  for (int i = threadIdx.x; i < SSIM_EXT * SSIM_TILE; i += SSIM_THREADS) {
    const int r = i / SSIM_TILE, c = i % SSIM_TILE;
    float x[11], y[11], p[11];
#pragma unroll
    for (int k = 0; k < 11; k++) { x[k] = s_x[r][c + k]; y[k] = s_y[r][c + k]; }
    s_h[0][r][c] = SSIM_TAPS(x, 0);
    s_h[1][r][c] = SSIM_TAPS(y, 0);
#pragma unroll
    for (int k = 0; k < 11; k++) p[k] = x[k] * y[k];
    s_h[4][r][c] = SSIM_TAPS(p, 0);
#pragma unroll
    for (int k = 0; k < 11; k++) { x[k] = x[k] * x[k]; y[k] = y[k] * y[k]; }
    s_h[2][r][c] = SSIM_TAPS(x, 0);
    s_h[3][r][c] = SSIM_TAPS(y, 0);
  }
  __syncthreads();
  const int tx = threadIdx.x % SSIM_TILE, ty = threadIdx.x / SSIM_TILE;
  float mu1[SSIM_ROWS_PER_THREAD], mu2[SSIM_ROWS_PER_THREAD], e11[SSIM_ROWS_PER_THREAD], e22[SSIM_ROWS_PER_THREAD], e12[SSIM_ROWS_PER_THREAD];
  ssim_columns(s_h[0], ty, tx, mu1);
  ssim_columns(s_h[1], ty, tx, mu2);
  ssim_columns(s_h[2], ty, tx, e11);
  ssim_columns(s_h[3], ty, tx, e22);
  ssim_columns(s_h[4], ty, tx, e12);
  const float C1 = (float)(0.01 * 0.01), C2 = (float)(0.03 * 0.03);
  const int gx = t.x0 + tx;
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < SSIM_ROWS_PER_THREAD; j++) {
    const int gy = t.y0 + ty * SSIM_ROWS_PER_THREAD + j;
    if (gy >= H || gx >= W) continue;
    const float mu1_sq = mu1[j] * mu1[j], mu2_sq = mu2[j] * mu2[j], mu12 = mu1[j] * mu2[j];
    const float s1 = e11[j] - mu1_sq, s2 = e22[j] - mu2_sq, s12 = e12[j] - mu12;
    const float A1 = 2.f * mu12 + C1, A2 = 2.f * s12 + C2, B1 = mu1_sq + mu2_sq + C1, B2 = s1 + s2 + C2;
    const float r1 = A1 / B1, r2 = A2 / B2, m = r1 * r2;
    sum += m;
    const int64_t at = base + (int64_t)gy * W + gx;
    if (map) map[at] = m;
    if (deriv) {
      const float mm = mu1[j] * m;
      deriv[at] = 2.f * ((mu2[j] * r2 - mm) / B1) + 2.f * ((mm - mu2[j] * r1) / B2);   // d_mu
      deriv[at + plane_stride_all] = -(m / B2);                                        // d_s1
      deriv[at + 2 * plane_stride_all] = 2.f * (r1 / B2);                              // d_s12
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}

// per image: the mean of m = (partials of its C * tiles workgroups, in index order) / (C H W); one workgroup per image
__global__ void __launch_bounds__(SSIM_THREADS)
ssim_finish_kernel(const float* __restrict__ partial, int64_t per_image, double count, float* __restrict__ mean) {
  __shared__ double s_red[SSIM_THREADS / 64];
  const float* p = partial + (int64_t)blockIdx.x * per_image;
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < per_image; i += SSIM_THREADS) acc += (double)p[i];
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 64);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) mean[blockIdx.x] = (float)(((s_red[0] + s_red[1]) + (s_red[2] + s_red[3])) / count);
}

__global__ void __launch_bounds__(SSIM_THREADS)
ssim_backward_kernel(const float* __restrict__ img1, const float* __restrict__ img2, const float* __restrict__ deriv,
                     int64_t plane_stride_all, const float* __restrict__ g_per_image, int planes_per_image, int H, int W, int tiles_x,
                     int tiles_y, float* __restrict__ g_img1) {
  __shared__ float s_d[3][SSIM_EXT][SSIM_EXT];
  __shared__ float s_h[3][SSIM_EXT][SSIM_TILE];
  const SsimTile t = ssim_tile(tiles_x, tiles_y);
  const int64_t base = t.plane * H * W;
#pragma unroll
  for (int q = 0; q < 3; q++) ssim_stage(deriv + q * plane_stride_all + base, H, W, t.y0, t.x0, s_d[q]);
  __syncthreads();
  for (int i = threadIdx.x; i < SSIM_EXT * SSIM_TILE; i += SSIM_THREADS) {
    const int r = i / SSIM_TILE, c = i % SSIM_TILE;
#pragma unroll
    for (int q = 0; q < 3; q++) {
      float v[11];
#pragma unroll
      for (int k = 0; k < 11; k++) v[k] = s_d[q][r][c + k];
      s_h[q][r][c] = SSIM_TAPS(v, 0);
    }
  }
  __syncthreads();
  const int tx = threadIdx.x % SSIM_TILE, ty = threadIdx.x / SSIM_TILE;
  float b_mu[SSIM_ROWS_PER_THREAD], b_s1[SSIM_ROWS_PER_THREAD], b_s12[SSIM_ROWS_PER_THREAD];
  ssim_columns(s_h[0], ty, tx, b_mu);
  ssim_columns(s_h[1], ty, tx, b_s1);
  ssim_columns(s_h[2], ty, tx, b_s12);
  // the image's mean has C H W terms: d mean / d m = 1 / (C H W), times what arrived for that mean
  const float s = g_per_image[t.plane / planes_per_image] / (float)((double)planes_per_image * H * W);
  const int gx = t.x0 + tx;
#pragma unroll
  for (int j = 0; j < SSIM_ROWS_PER_THREAD; j++) {
    const int gy = t.y0 + ty * SSIM_ROWS_PER_THREAD + j;
    if (gy >= H || gx >= W) continue;
    const int64_t at = base + (int64_t)gy * W + gx;
    const float x = img1[at], y = img2[at];
    g_img1[at] = s * (b_mu[j] + ((2.f * x) * b_s1[j] + y * b_s12[j]));
  }
}

// tiles of the whole batch; 0 when the shape is not launchable (an empty or negative dimension, more than 2^31 - 1 workgroups)
static int64_t ssim_blocks(int32_t N, int32_t C, int32_t H, int32_t W, int* tiles_x, int* tiles_y) {
  if (N < 1 || C < 1 || H < 1 || W < 1) return 0;
  const int64_t tx = ((int64_t)W + SSIM_TILE - 1) / SSIM_TILE, ty = ((int64_t)H + SSIM_TILE - 1) / SSIM_TILE;
  if (tx * ty > INT32_MAX || (int64_t)N * C > INT32_MAX) return 0;
  const int64_t blocks = (int64_t)N * C * tx * ty;
  if (blocks / (tx * ty) != (int64_t)N * C || blocks > INT32_MAX) return 0;
  *tiles_x = (int)tx;
  *tiles_y = (int)ty;
  return blocks;
}

extern "C" size_t gip_ssim_workspace_bytes(int32_t N, int32_t C, int32_t H, int32_t W) {
  int tx, ty;
  return (size_t)ssim_blocks(N, C, H, W, &tx, &ty) * sizeof(float);
}

extern "C" int gip_ssim_forward(const float* img1, const float* img2, int32_t N, int32_t C, int32_t H, int32_t W, float* per_image_mean,
                                float* deriv, float* map, void* workspace, void* stream) {
  int tx, ty;
  const int64_t blocks = ssim_blocks(N, C, H, W, &tx, &ty);
  if (!img1 || !img2 || !per_image_mean || !workspace || blocks == 0) return 1;
  const int64_t all = (int64_t)N * C * H * W;
  hipLaunchKernelGGL(ssim_forward_kernel, dim3((unsigned)blocks), dim3(SSIM_THREADS), 0, (hipStream_t)stream, img1, img2, (int)H, (int)W, tx,
                     ty, deriv, all, map, (float*)workspace);
  hipLaunchKernelGGL(ssim_finish_kernel, dim3((unsigned)N), dim3(SSIM_THREADS), 0, (hipStream_t)stream, (const float*)workspace,
                     blocks / N, (double)C * H * W, per_image_mean);
  return hipGetLastError() == hipSuccess ? 0 : 3;
}

extern "C" int gip_ssim_backward(const float* img1, const float* img2, const float* deriv, const float* g_per_image, int32_t N, int32_t C,
                                 int32_t H, int32_t W, float* g_img1, void* stream) {
  int tx, ty;
  const int64_t blocks = ssim_blocks(N, C, H, W, &tx, &ty);
  if (!img1 || !img2 || !deriv || !g_per_image || !g_img1 || blocks == 0) return 1;
  hipLaunchKernelGGL(ssim_backward_kernel, dim3((unsigned)blocks), dim3(SSIM_THREADS), 0, (hipStream_t)stream, img1, img2, deriv,
                     (int64_t)N * C * H * W, g_per_image, (int)C, (int)H, (int)W, tx, ty, g_img1);
  return hipGetLastError() == hipSuccess ? 0 : 3;
}
