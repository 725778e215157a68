// volume_common.h — what the two volume-rendering kernel files share (the density renderer and volume_sdf.hip, the NeuS renderer of a
// signed-distance field): the assignment of one wave to a ray, the definition's min and max (volume_sdf.hip writes its relu and clip
// with them), the doubling sum over the 64 lanes (the density weights'), the butterfly sum that ends every per-ray accumulation, and
// the host's limits.  Device functions are inlined and host functions static, as in mesh_common.h, which this header builds on.
#pragma once
#include "mesh_common.h"

#define VOL_RAYS_PER_BLOCK (MESH_THREADS / 64)
#define VOL_MAX_CHANNELS 16

__device__ __forceinline__ float vol_min(float a, float b) { return b < a ? b : a; }
__device__ __forceinline__ float vol_max(float a, float b) { return b > a ? b : a; }

// the doubling scan of the definition over the 64 lanes, towards higher lanes (UP) or towards lower ones
template <bool UP>
__device__ __forceinline__ float vol_scan(float s, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const float y = UP ? __shfl_up(s, d, 64) : __shfl_down(s, d, 64);
    if (UP ? lane >= d : lane + d < 64) s += y;
  }
  return s;
}

// the sum over the 64 lanes by the xor butterfly 32, 16, .. 1: every lane ends with the same total
__device__ __forceinline__ float vol_wave_sum(float v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// ------------------------------------------------------------------------------------------------------------------------ host
// workgroups of one wave per ray; 0 when the count is not launchable
static int64_t vol_ray_blocks(int64_t R) {
  if (R < 1 || R > INT32_MAX / 64) return 0;
  return (R + VOL_RAYS_PER_BLOCK - 1) / VOL_RAYS_PER_BLOCK;
}

static bool vol_rows_ok(int64_t R, int64_t M) { return R >= 0 && R <= INT32_MAX / 64 && mesh_count_ok(M); }
