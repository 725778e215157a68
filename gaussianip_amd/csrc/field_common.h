// field_common.h — what field.hip (the density field on the grid), field_sample.hip (the field at query points) and texture.hip (the
// field at the texels of an atlas) share: the prepared form of the Gaussians, the limits of the shapes, the workspace, and the ONE walk
// of a workgroup over the members of its block.  All three are compiled with -ffp-contract=off; every device function here is inlined.
//
// Prepared form (field_prepare_kernel in field.hip, launched through field_prepare_launch): per Gaussian a record of FIELD_REC floats —
// xyz' (3), the six terms a b c d e f of the adjugate inverse of Sigma with 1 / (det + 1e-24), opacity — and one 64-bit range word of
// six 10-bit fields, (first, last) block per axis of the interval of blocks the centre belongs to, "empty" = first > last.  The
// workspace holds the records [P, 10] and then the range words [P] (8-byte aligned: 40 P is a multiple of 8).
//
// The walk (field_walk): the workgroup of block (bx, by, bz) walks the P range words (8 bytes per Gaussian, the same L2-resident table
// for all workgroups), FIELD_CHUNK per trip, and compacts the members IN INDEX ORDER (ballot + popcount, per-wave counts through a
// double-buffered LDS table, one barrier per trip) into an LDS index list of FIELD_CAP; when a further trip might overflow the list, and
// at the end, the listed records are staged in LDS FIELD_BATCH at a time (pre-scaled by -0.5 and -1, exact; with the Gaussian's rgb when
// asked) and every lane evaluates them against its N points in registers.  A pair is evaluated once — d = x - mu', the halves t0, t1, t2
// of -A d / 2, power = -0.5 d^T A d as an explicit fmaf chain, e = exp(power) with a positive power counting as 0 (__expf, v_exp_f32,
// unless FIELD_PRECISE_EXP) — and handed to the kernel's own callable, which adds its sums.  Each batch is summed on its own and then
// added to the point's totals (a two-level sum: the rounding error grows with sqrt(256) + sqrt(batches) instead of sqrt(members)).
// The per-point order is the Gaussians' order in memory whatever the schedule: no float atomic, two runs are bitwise equal, and two
// kernels that hand the walk the same point and block get the same `power` and `e`, bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gip_model.h"

#define FIELD_THREADS 256
#define FIELD_WAVES (FIELD_THREADS / 64)
#define FIELD_SUB 4                                 // range words tested per thread per trip
#define FIELD_CHUNK (FIELD_THREADS * FIELD_SUB)     // 1024
#define FIELD_CAP 2048                              // capacity of the LDS member list; flushed when a trip might overflow it
#define FIELD_BATCH 256                             // records staged in LDS at a time
#define FIELD_REC 10                                // floats of a record
#define FIELD_MAX_BLOCKS 1024                       // per axis: the range word has 10 bits per field

// ------------------------------------------------------------------------------------------------------------------ host side
static inline int field_shape_ok(int64_t P, int32_t R, int32_t nb) {
  if (P < 0 || P > INT32_MAX || R < 1 || nb < 1 || nb > FIELD_MAX_BLOCKS || R % nb != 0) return 0;
  if ((int64_t)nb * nb * nb > INT32_MAX) return 0;
  return 1;
}

// the three gip_*_workspace_size entry points
static inline int field_workspace_size(int64_t P, int32_t R, int32_t nb, size_t* bytes) {
  if (!bytes || !field_shape_ok(P, R, nb)) return 1;
  *bytes = (size_t)P * (FIELD_REC * sizeof(float) + sizeof(uint64_t));
  return 0;
}

struct FieldPrepared {
  float* rec;
  uint64_t* range;
};

static inline FieldPrepared field_workspace_split(void* workspace, int64_t P) {
  float* rec = (float*)workspace;
  return {rec, (uint64_t*)(rec + (size_t)P * FIELD_REC)};
}

// field.hip: fills `out` for P > 0 Gaussians on `stream` (a host function, so the other two files need no kernel of their own)
__attribute__((visibility("hidden"))) void field_prepare_launch(const float* xyz, const float* opacity, const float* scaling,
                                                                const float* rotation, int64_t P, const float* center, float scale,
                                                                const float* grid, int R, int nb, float margin, FieldPrepared out,
                                                                hipStream_t stream);

// ------------------------------------------------------------------------------------------------------------------ device side
template <bool RGB>
struct FieldLds {
  int idx[FIELD_CAP];
  float4 rec[FIELD_BATCH][RGB ? 4 : 3];
  int cnt[2][FIELD_SUB][FIELD_WAVES];
};

// one point against one Gaussian
struct FieldPair {
  float4 c0, c1, c2, c3;   // (xyz', opacity), (-A/2, -B, -C, -D/2), (-E, -F/2, 0, 0), (rgb, 0) or zeros
  float dx, dy, dz;        // point - xyz'
  float t0, t1, t2;        // -(A/2 dx + B dy + C dz), -(D/2 dy + E dz), -(F/2 dz)
  float power, e;          // power = dx t0 + dy t1 + dz t2; e = exp(power), 0 for a positive power
};

// Adds, for k < slots (workgroup-uniform; the points of slots >= `slots` are not evaluated), the sums of point (px[k], py[k], pz[k])
// over the members of block (bx, by, bz) to acc[k]: add(pair, part) adds one pair to the S batch sums of its point.  Every thread of
// the workgroup calls it; it ends with a barrier, so it may be called again.
template <int N, int S, bool RGB, typename Add>
__device__ __forceinline__ void field_walk(FieldLds<RGB>& lds, const float* __restrict__ rec, const uint64_t* __restrict__ range,
                                           const float* __restrict__ rgb, int64_t P, int bx, int by, int bz, const float (&px)[N],
                                           const float (&py)[N], const float (&pz)[N], int slots, float (&acc)[N][S], Add add) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint64_t lt = lane ? (~0ull >> (64 - lane)) : 0ull;   // lanes below this one
  int staged = 0, par = 0;
  for (int64_t base = 0; base < P; base += FIELD_CHUNK) {
    // ---- which of the next 1024 Gaussians belong to this block; their indices appended to lds.idx in index order
    uint64_t bal[FIELD_SUB];
    bool mine[FIELD_SUB];
#pragma unroll
    for (int i = 0; i < FIELD_SUB; i++) {
      const int64_t g = base + i * FIELD_THREADS + tid;
      bool m = false;
      if (g < P) {
        const uint64_t w = range[g];
        const int x0 = (int)(w & 1023), x1 = (int)((w >> 10) & 1023), y0 = (int)((w >> 20) & 1023), y1 = (int)((w >> 30) & 1023),
                  z0 = (int)((w >> 40) & 1023), z1 = (int)((w >> 50) & 1023);
        m = bx >= x0 && bx <= x1 && by >= y0 && by <= y1 && bz >= z0 && bz <= z1;
      }
      mine[i] = m;
      bal[i] = __ballot(m);
      if (lane == 0) lds.cnt[par][i][wave] = __popcll(bal[i]);
    }
    __syncthreads();
    int run = staged;
#pragma unroll
    for (int i = 0; i < FIELD_SUB; i++) {
      int off = 0;
#pragma unroll
      for (int w = 0; w < FIELD_WAVES; w++) {
        if (w == wave) off = run;
        run += lds.cnt[par][i][w];
      }
      if (mine[i]) lds.idx[off + __popcll(bal[i] & lt)] = (int)(base + i * FIELD_THREADS + tid);
    }
    staged = run;   // the same value in every thread; <= FIELD_CAP because a flush leaves at most FIELD_CAP - FIELD_CHUNK behind
    par ^= 1;
    if (staged <= FIELD_CAP - FIELD_CHUNK && base + FIELD_CHUNK < P) continue;
    // ---- flush: add the listed Gaussians to this lane's points, 256 records at a time
    for (int sb = 0; sb < staged; sb += FIELD_BATCH) {
      __syncthreads();   // lds.idx is complete; the previous batch's records are no longer read
      const int n = min(FIELD_BATCH, staged - sb);
      if (tid < n) {
        const int64_t gi = lds.idx[sb + tid];
        const float* r = rec + gi * FIELD_REC;
        // power = dx (A dx + B dy + C dz) + dy (D dy + E dz) + dz (F dz): the scalings by -0.5 and -1 are exact
        lds.rec[tid][0] = make_float4(r[0], r[1], r[2], r[9]);
        lds.rec[tid][1] = make_float4(-0.5f * r[3], -r[4], -r[5], -0.5f * r[6]);
        lds.rec[tid][2] = make_float4(-r[7], -0.5f * r[8], 0.f, 0.f);
        if (RGB) lds.rec[tid][3] = make_float4(rgb[gi * 3], rgb[gi * 3 + 1], rgb[gi * 3 + 2], 0.f);
      }
      __syncthreads();
      float part[N][S];
#pragma unroll
      for (int k = 0; k < N; k++)
#pragma unroll
        for (int c = 0; c < S; c++) part[k][c] = 0.f;
      for (int j = 0; j < n; j++) {
        FieldPair q;
        q.c0 = lds.rec[j][0], q.c1 = lds.rec[j][1], q.c2 = lds.rec[j][2];
        q.c3 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (RGB) q.c3 = lds.rec[j][3];
#pragma unroll
        for (int k = 0; k < N; k++) {
          if (k >= slots) continue;
          q.dx = px[k] - q.c0.x, q.dy = py[k] - q.c0.y, q.dz = pz[k] - q.c0.z;
          q.t0 = fmaf(q.c1.z, q.dz, fmaf(q.c1.y, q.dy, q.c1.x * q.dx));
          q.t1 = fmaf(q.c2.x, q.dz, q.c1.w * q.dy);
          q.t2 = q.c2.y * q.dz;
          q.power = fmaf(q.dx, q.t0, fmaf(q.dy, q.t1, q.dz * q.t2));
#ifdef FIELD_PRECISE_EXP
          q.e = q.power > 0.f ? 0.f : expf(q.power);
#else
          q.e = q.power > 0.f ? 0.f : __expf(q.power);
#endif
          add(q, part[k]);
        }
      }
#pragma unroll
      for (int k = 0; k < N; k++)
#pragma unroll
        for (int c = 0; c < S; c++) acc[k][c] += part[k][c];
    }
    staged = 0;
  }
  __syncthreads();   // a further call reuses lds.idx and lds.cnt
}
