// fold_check.hip — the backward blend's two fold networks (gaussianip_amd/csrc/bwd_fold.h) on the same inputs: the
// v_permlane32/16_swap network and the LDS-crossbar network must leave the same BITS in every lane the row store reads
// (lanes 16 r + 0..4: all twenty sums of a pair), NaNs in the same places.  Exits non-zero on the first difference.
//
// 4096 accumulator sets (20 registers x 64 lanes each), one wave per set, in four classes of 1024:
//   0  normal values in [-1, 1)                       1  magnitudes mixed from 1e-30 to 1e30, either sign
//   2  +-0, denormals, +-inf among normal values      3  entry B all +0 (the odd tail of a list), entry A as class 0 / 1
// `fold_check time` also times both networks (R folds per wave, five waves per SIMD), for the A/B in profiles/.
//
// build: hipcc --offload-arch=gfx950 -O3 -I gaussianip_amd/csrc -o fold_check tools/micro/fold_check.hip
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "bwd_fold.h"

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)

static const int SETS = 4096;

__device__ __forceinline__ void load_acc(BwdAcc& a, const float* p) {
  a.v0 = p[0]; a.v1 = p[64]; a.v2 = p[128]; a.v3 = p[192]; a.v4 = p[256]; a.v5 = p[320]; a.v6 = p[384]; a.v7 = p[448];
  a.v8 = p[512]; a.v9 = p[576];
}

// in: [sets][20][64] (entry A's ten terms, then entry B's); out_swap, out_xbar: [sets][64], the register the store reads
__global__ void __launch_bounds__(64) check_kernel(const float* __restrict__ in, uint32_t* __restrict__ out_swap,
                                                   uint32_t* __restrict__ out_xbar, int sets) {
  const int lane = threadIdx.x, set = blockIdx.x;
  if (set >= sets) return;                               // wave-uniform
  const float* p = in + (size_t)set * 1280 + lane;
  BwdAcc a, b, c, d;
  load_acc(a, p); load_acc(b, p + 640);
  c = a; d = b;
  fold_two_entries_swap(a, b);
  fold_two_entries(c, d, (lane ^ 32) << 2);
  out_swap[(size_t)set * 64 + lane] = __float_as_uint(b.v8);
  out_xbar[(size_t)set * 64 + lane] = __float_as_uint(d.v8);
}

template <int NET>
__global__ void __launch_bounds__(256) time_kernel(float* __restrict__ sink, int R, float seed) {
  const int lane = threadIdx.x & 63;
  const float s = seed + lane * 1e-3f;
  BwdAcc a = {s, s + 1, s + 2, s + 3, s + 4, s + 5, s + 6, s + 7, s + 8, s + 9}, b = a;
  float acc = 0.f;
  for (int r = 0; r < R; r++) {
    if (NET) fold_two_entries(a, b, (lane ^ 32) << 2); else fold_two_entries_swap(a, b);
    acc += b.v8;
    b.v8 = a.v8 = acc * 1e-3f;                           // the next fold depends on this one's result
  }
  if (acc == 123.456f) sink[0] = acc;                    // never true
}

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (uint32_t)(g_rng >> 32); }
static float uni() { return (float)(rnd() >> 8) * (1.0f / 16777216.0f); }   // [0, 1)
static float normal_value() { return 2.f * uni() - 1.f; }
static float mixed_value() { const float m = powf(10.f, 60.f * uni() - 30.f); return rnd() & 1 ? m : -m; }
static float special_value() {
  uint32_t bits;
  switch (rnd() % 10) {
    case 0: bits = 0x00000000u; break;                           // +0
    case 1: bits = 0x80000000u; break;                           // -0
    case 2: bits = 1u + rnd() % 0x7fffffu; break;                // +denormal
    case 3: bits = 0x80000000u | (1u + rnd() % 0x7fffffu); break;
    case 4: bits = rnd() % 64 ? 0x00000001u : 0x7f800000u; break;   // +inf now and then (inf + -inf gives the NaNs)
    case 5: bits = rnd() % 64 ? 0x80000001u : 0xff800000u; break;
    default: return normal_value();
  }
  float f; memcpy(&f, &bits, 4); return f;
}

static const char* NETS[2] = {"swap", "crossbar"};

// the crossbar network against the swap network on the inputs at d_in (h: their host copy); 0 = equal
static int check(int net, const std::vector<float>& h, const float* d_in, uint32_t* d_a, uint32_t* d_b) {
  CHECK(hipMemset(d_a, 0xff, (size_t)SETS * 64 * 4)); CHECK(hipMemset(d_b, 0x55, (size_t)SETS * 64 * 4));
  hipLaunchKernelGGL(check_kernel, dim3(SETS), dim3(64), 0, 0, d_in, d_a, d_b, SETS);
  CHECK(hipGetLastError()); CHECK(hipDeviceSynchronize());
  std::vector<uint32_t> ra((size_t)SETS * 64), rb((size_t)SETS * 64);
  CHECK(hipMemcpy(ra.data(), d_a, ra.size() * 4, hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(rb.data(), d_b, rb.size() * 4, hipMemcpyDeviceToHost));
  long sums = 0, nans = 0, nonzero = 0;
  for (int s = 0; s < SETS; s++)
    for (int lane = 0; lane < 64; lane++) {
      if ((lane & 15) > 4) continue;                     // not a lane the row store reads
      const uint32_t x = ra[(size_t)s * 64 + lane], y = rb[(size_t)s * 64 + lane];
      const bool xn = (x & 0x7fffffffu) > 0x7f800000u, yn = (y & 0x7fffffffu) > 0x7f800000u;
      sums++; nans += xn; nonzero += (x & 0x7fffffffu) != 0;
      if (xn != yn || (!xn && x != y)) {
        const int r = lane >> 4, j = lane & 15, term = j < 4 ? 2 * j + (r & 1) : 8 + (r & 1);
        printf("DIFFERENT: set %d (class %d) lane %d (entry %c term %d): swap 0x%08x %s 0x%08x\n", s, s / (SETS / 4), lane,
               r >> 1 ? 'B' : 'A', term, x, NETS[net], y);
        return 1;
      }
    }
  // a fold that returned its input or zeros everywhere would pass the comparison: the sums must be live, and class 3's
  // entry B must be the exact +0 rows
  for (int s = 3 * SETS / 4; s < SETS; s++)
    for (int lane = 32; lane < 64; lane++)
      if ((lane & 15) <= 4 && rb[(size_t)s * 64 + lane] != 0u) { printf("DIFFERENT: set %d lane %d: all-zero entry B folds to 0x%08x\n", s, lane, rb[(size_t)s * 64 + lane]); return 1; }
  if (nonzero < sums / 2) { printf("DIFFERENT: only %ld of %ld sums are non-zero\n", nonzero, sums); return 1; }
  // set 0 against the plain sum in double, to tie the networks to the quantity they compute (class 0: no cancellation trouble)
  const float* p = h.data();
  for (int e = 0; e < 2; e++)
    for (int t = 0; t < 10; t++) {
      double ref = 0, mag = 0;
      for (int l = 0; l < 64; l++) { ref += p[(e * 10 + t) * 64 + l]; mag += fabs(p[(e * 10 + t) * 64 + l]); }
      const int lane = 32 * e + 16 * (t & 1) + (t < 8 ? t >> 1 : 4);
      float got; memcpy(&got, &rb[lane], 4);
      if (fabs(got - ref) > 64 * 6e-8 * mag) { printf("DIFFERENT: set 0 entry %d term %d: fold %.9g, sum %.9g\n", e, t, got, ref); return 1; }
    }
  printf("{\"fold_check\": \"equal\", \"network\": \"%s\", \"against\": \"swap\", \"sets\": %d, \"sums_compared\": %ld, \"nan_sums\": %ld}\n",
         NETS[net], SETS, sums, nans);
  return 0;
}

int main(int argc, char** argv) {
  std::vector<float> h((size_t)SETS * 1280);
  for (int s = 0; s < SETS; s++) {
    const int cls = s / (SETS / 4);
    float* p = h.data() + (size_t)s * 1280;
    for (int i = 0; i < 1280; i++) {
      if (cls == 0) p[i] = normal_value();
      else if (cls == 1) p[i] = mixed_value();
      else if (cls == 2) p[i] = special_value();
      else p[i] = i >= 640 ? 0.f : (s & 1 ? mixed_value() : normal_value());
    }
  }
  float* d_in; uint32_t *d_a, *d_b;
  CHECK(hipMalloc(&d_in, h.size() * 4)); CHECK(hipMalloc(&d_a, (size_t)SETS * 64 * 4)); CHECK(hipMalloc(&d_b, (size_t)SETS * 64 * 4));
  CHECK(hipMemcpy(d_in, h.data(), h.size() * 4, hipMemcpyHostToDevice));
  if (int rc = check(1, h, d_in, d_a, d_b)) return rc;

  if (argc > 1 && !strcmp(argv[1], "time")) {
    const int R = 4096, grid = 256 * 5;                  // 256-thread workgroups, one wave per SIMD each, five per CU
    float* d_sink; CHECK(hipMalloc(&d_sink, 64));
    for (int net = 0; net < 2; net++) {
      float best = 1e30f;
      for (int rep = 0; rep < 5; rep++) {
        hipEvent_t e0, e1; CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
        CHECK(hipEventRecord(e0));
        if (net == 1) hipLaunchKernelGGL(time_kernel<1>, dim3(grid), dim3(256), 0, 0, d_sink, R, 1.f + rep);
        else hipLaunchKernelGGL(time_kernel<0>, dim3(grid), dim3(256), 0, 0, d_sink, R, 1.f + rep);
        CHECK(hipEventRecord(e1)); CHECK(hipEventSynchronize(e1));
        float ms; CHECK(hipEventElapsedTime(&ms, e0, e1));
        if (ms < best) best = ms;
        CHECK(hipEventDestroy(e0)); CHECK(hipEventDestroy(e1));
      }
      // per fold and SIMD: launch time x 2.4 GHz over the folds each of the 1024 SIMDs ran (five waves x R)
      printf("{\"network\": \"%s\", \"waves_per_simd\": 5, \"folds_per_wave\": %d, \"launch_ms\": %.4f, \"simd_cycles_per_fold_at_2.4GHz\": %.1f}\n",
             NETS[net], R, best, best * 1e-3 * 2.4e9 / (5.0 * R));
    }
  }
  return 0;
}
