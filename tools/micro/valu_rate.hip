// valu_rate.hip — issue rate of wave64 fp32 vector instructions on gfx950 by waves per SIMD.
//
// Question: does one SIMD retire a wave64 v_fma_f32 every 4 cycles (what `roofline_valu` assumed in round 2, from
// SQ_ACTIVE_INST_VALU / SQ_INSTS_VALU = 4.18 on the render kernels) or every 2 cycles once >= 2 waves share the SIMD
// (the guide's constants table: "v_fma_f32 (wave64) 2 cyc (SIMD-32); one wave alone: 4")?
//
// Method: every wave runs R x 64 INDEPENDENT instructions (16 accumulator chains, dependent distance 16) between two
// s_memtime stamps.  k waves per SIMD are made co-resident as workgroups of 256 * min(k, 4) threads, k / min(k, 4) of
// them per CU (grid = 256 CUs x that).  Per wave: cycles / instruction = dt / (R * 64); the SIMD's issue interval per
// wave-instruction is that divided by the k waves that share it (they overlap in time: start skew is printed).
// The clock is dt(s_memtime) / dt(s_memrealtime at 100 MHz).  Forms: v_fma_f32, v_pk_fma_f32 (two lanes' worth per
// instruction), v_exp_f32 (transcendental), and a render-like mix (3 fma : 1 mul : 1 cndmask : 1 exp per 6).
//
//
// Lane exchanges (`./valu_rate xchg`): what one cross-lane exchanged term costs the SIMD, for the blend kernels' folds.
//   swap32 / swap16        s_nop 1, v_permlane32/16_swap_b32, s_nop 1 (the hazard padding the kernels carry), one per unit
//   swap32_run / swap16_run  s_nop 1, then eight swaps back to back (how the backward's fold issues a level)
//   dpp_quad_perm / dpp_row_ror8   v_add_f32_dpp, the move and the add in one instruction
//   xbar32    the LDS-crossbar form of one exchanged term at lane ^ 32: two v_cndmask on an SGPR lane mask, one
//             ds_bpermute_b32, one v_add_f32; ten independent exchanges are issued, then ONE s_waitcnt lgkmcnt(0), then the adds
//   xbar16    the same at lane ^ 16 with ds_swizzle_b32 swizzle(SWAP,16)
// Each runs alone at 1, 2, 4, 5 and 7 waves per SIMD, and with 8 or 16 independent v_fma_f32 after every exchange: a cost
// that blocks the SIMD stays on top of the fma stream's time, a latency private to the wave hides under it.
// 5 and 7 waves per SIMD: 256-thread workgroups (one wave per SIMD), capped to k per CU by their dynamic LDS size.
//
// build: hipcc --offload-arch=gfx950 -O3 -o valu_rate valu_rate.hip      run: ./valu_rate > profiles/r03_valu_rate.txt
//                                                                             ./valu_rate xchg > profiles/lane_exchange_rate.txt
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>

typedef float v2f __attribute__((ext_vector_type(2)));

#define REP16(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15)

enum { FMA = 0, PKFMA = 1, EXP = 2, MIX = 3 };

template <int KIND>
__global__ void __launch_bounds__(1024) rate_kernel(unsigned long long* __restrict__ stamps, float* __restrict__ sink, int R, float seed) {
  float a[16];
  v2f p[16];
#pragma unroll
  for (int i = 0; i < 16; i++) {
    a[i] = seed + i + threadIdx.x * 1e-3f;
    if constexpr (KIND == PKFMA) p[i] = (v2f){a[i], a[i] + 0.5f}; else p[i] = (v2f){0.f, 0.f};
  }
  const float b = 0.999f + seed * 1e-6f, c = 1e-3f;
  const v2f pb = (v2f){b, b}, pc = (v2f){c, c};
  __syncthreads();
  const unsigned long long t0 = __builtin_amdgcn_s_memtime();
  const unsigned long long r0 = __builtin_amdgcn_s_memrealtime();
  for (int r = 0; r < R; r++) {
#pragma unroll
    for (int u = 0; u < 4; u++) {
      if constexpr (KIND == FMA) {
#define X(i) asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(a[i]) : "v"(b), "v"(c));
        REP16(X)
#undef X
      } else if constexpr (KIND == PKFMA) {
#define X(i) asm volatile("v_pk_fma_f32 %0, %0, %1, %2" : "+v"(p[i]) : "v"(pb), "v"(pc));
        REP16(X)
#undef X
      } else if constexpr (KIND == EXP) {
#define X(i) asm volatile("v_exp_f32 %0, %0" : "+v"(a[i]));
        REP16(X)
#undef X
      } else {
        // 16 instructions: per group of 6 -> fma fma fma mul cndmask exp (the blend's rough mix), independent registers
        asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(a[0]) : "v"(b), "v"(c));
        asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(a[1]) : "v"(b), "v"(c));
        asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(a[2]) : "v"(b), "v"(c));
        asm volatile("v_mul_f32 %0, %0, %1" : "+v"(a[3]) : "v"(b));
        asm volatile("v_cndmask_b32 %0, %0, %1, vcc" : "+v"(a[4]) : "v"(b));
        asm volatile("v_exp_f32 %0, %0" : "+v"(a[5]));
        asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(a[6]) : "v"(b), "v"(c));
        asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(a[7]) : "v"(b), "v"(c));
        asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(a[8]) : "v"(b), "v"(c));
        asm volatile("v_mul_f32 %0, %0, %1" : "+v"(a[9]) : "v"(b));
        asm volatile("v_cndmask_b32 %0, %0, %1, vcc" : "+v"(a[10]) : "v"(b));
        asm volatile("v_exp_f32 %0, %0" : "+v"(a[11]));
        asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(a[12]) : "v"(b), "v"(c));
        asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(a[13]) : "v"(b), "v"(c));
        asm volatile("v_mul_f32 %0, %0, %1" : "+v"(a[14]) : "v"(b));
        asm volatile("v_max_f32 %0, %0, %1" : "+v"(a[15]) : "v"(c));
      }
    }
  }
  const unsigned long long t1 = __builtin_amdgcn_s_memtime();
  const unsigned long long r1 = __builtin_amdgcn_s_memrealtime();
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 16; i++) s += KIND == PKFMA ? p[i][0] + p[i][1] : a[i];
  if (s == 123.456f) sink[0] = s;                      // keeps the chains live; never true
  if ((threadIdx.x & 63) == 0) {
    const size_t w = (size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    stamps[4 * w + 0] = t0; stamps[4 * w + 1] = t1; stamps[4 * w + 2] = r0; stamps[4 * w + 3] = r1;
  }
}

template <int KIND>
static void run(const char* name, int k, unsigned long long* d_st, float* d_sink) {
  const int cus = 256, wg_waves_per_simd = std::min(k, 4), threads = 256 * wg_waves_per_simd, wgs_per_cu = k / wg_waves_per_simd;
  const int grid = cus * wgs_per_cu, waves = grid * threads / 64, R = 4096;
  std::vector<unsigned long long> h(4 * (size_t)waves);
  double best_cyc = 1e30, best_clock = 0, best_span = 0, best_ms = 0;
  int occ_blocks = 0;
  hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ_blocks, rate_kernel<KIND>, threads, 0);
  const int resident_waves_per_simd = std::min(occ_blocks, wgs_per_cu) * threads / 256;
  for (int rep = 0; rep < 5; rep++) {
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    hipEventRecord(e0);
    hipLaunchKernelGGL(rate_kernel<KIND>, dim3(grid), dim3(threads), 0, 0, d_st, d_sink, R, 1.0f + rep);
    hipEventRecord(e1); hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1);
    hipMemcpy(h.data(), d_st, h.size() * 8, hipMemcpyDeviceToHost);
    std::vector<double> cyc(waves);
    double clk = 0; unsigned long long tmin = ~0ull, tmax0 = 0;
    for (int w = 0; w < waves; w++) {
      cyc[w] = double(h[4 * w + 1] - h[4 * w]) / (double(R) * 64.0);
      clk += double(h[4 * w + 1] - h[4 * w]) / (double(h[4 * w + 3] - h[4 * w + 2]) * 10.0);   // cycles per ns -> GHz (realtime = 100 MHz)
      if (w < threads / 64) { tmin = std::min(tmin, h[4 * w]); tmax0 = std::max(tmax0, h[4 * w]); }   // start skew inside workgroup 0
    }
    std::sort(cyc.begin(), cyc.end());
    const double med = cyc[waves / 2];
    if (med < best_cyc) { best_cyc = med; best_clock = clk / waves; best_span = double(tmax0 - tmin); best_ms = ms; }
    hipEventDestroy(e0); hipEventDestroy(e1);
  }
  const double lanes_per_instr = KIND == PKFMA ? 128.0 : 64.0;
  // cross-check from the launch's wall time: total wave-instructions / (1024 SIMDs x cycles of the launch at the measured clock)
  const double wall_cyc = best_ms * 1e-3 * best_clock * 1e9;
  const double simd_cyc_wall = wall_cyc / (double(waves) * R * 64.0 / 1024.0);
  printf("{\"instr\": \"%s\", \"waves_per_simd_launched\": %d, \"waves_per_simd_resident\": %d, \"workgroup\": %d, \"grid\": %d, "
         "\"cycles_per_instr_per_wave\": %.3f, \"simd_cycles_per_wave_instr\": %.3f, \"simd_cycles_per_wave_instr_from_wall\": %.3f, "
         "\"lane_ops_per_simd_cycle\": %.2f, \"clock_ghz\": %.3f, \"start_skew_cycles_wg0\": %.0f, \"launch_ms\": %.3f}\n",
         name, k, resident_waves_per_simd, threads, grid, best_cyc, best_cyc / resident_waves_per_simd, simd_cyc_wall,
         lanes_per_instr * resident_waves_per_simd / best_cyc, best_clock, best_span, best_ms);
}

// ---- lane exchanges ----
enum { SWAP32 = 0, SWAP16 = 1, SWAP32_RUN = 2, SWAP16_RUN = 3, DPP_QP = 4, DPP_ROR = 5, XBAR32 = 6, XBAR16 = 7, FMA_ONLY = 8 };
__host__ __device__ constexpr int xchg_units(int kind) { return kind == XBAR32 || kind == XBAR16 ? 10 : kind == DPP_QP || kind == DPP_ROR ? 16 : 8; }

// FM independent fma after exchange unit u (sixteen chains, dependent distance 16)
template <int FM>
__device__ __forceinline__ void fma_fill(float (&f)[16], int u, float b, float c) {
#pragma unroll
  for (int j = 0; j < FM; j++) asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(f[(u * FM + j) & 15]) : "v"(b), "v"(c));
}

template <int KIND, int FM>
__global__ void __launch_bounds__(1024) xchg_kernel(unsigned long long* __restrict__ stamps, float* __restrict__ sink, int R, float seed) {
  float a[16], f[16], y[10], kp[10], sd[10];
#pragma unroll
  for (int i = 0; i < 16; i++) { a[i] = seed + i + threadIdx.x * 1e-3f; f[i] = a[i] * 0.5f; }
#pragma unroll
  for (int i = 0; i < 10; i++) { y[i] = seed * 0.25f + i + threadIdx.x * 2e-3f; kp[i] = sd[i] = 0.f; }
  const float b = 0.999f + seed * 1e-6f, c = 1e-3f;
  const unsigned long long m32 = 0xffffffffull, m16 = 0x0000ffff0000ffffull;
  const int addr = ((threadIdx.x & 63) ^ 32) << 2;
  __syncthreads();
  const unsigned long long t0 = __builtin_amdgcn_s_memtime();
  const unsigned long long r0 = __builtin_amdgcn_s_memrealtime();
  for (int r = 0; r < R; r++) {
    if constexpr (KIND == FMA_ONLY) {
#pragma unroll
      for (int u = 0; u < 8; u++) fma_fill<FM>(f, u, b, c);
    } else if constexpr (KIND == SWAP32 || KIND == SWAP16) {
#pragma unroll
      for (int u = 0; u < 8; u++) {
        if constexpr (KIND == SWAP32) asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a[2 * u]), "+v"(a[2 * u + 1]));
        else asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a[2 * u]), "+v"(a[2 * u + 1]));
        fma_fill<FM>(f, u, b, c);
      }
    } else if constexpr (KIND == SWAP32_RUN || KIND == SWAP16_RUN) {
#define RUN8(OP) asm volatile("s_nop 1\n\t" OP " %0, %1\n\t" OP " %2, %3\n\t" OP " %4, %5\n\t" OP " %6, %7\n\t" OP " %8, %9\n\t" \
                              OP " %10, %11\n\t" OP " %12, %13\n\t" OP " %14, %15\n\ts_nop 1"                                      \
                              : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7]),     \
                                "+v"(a[8]), "+v"(a[9]), "+v"(a[10]), "+v"(a[11]), "+v"(a[12]), "+v"(a[13]), "+v"(a[14]), "+v"(a[15]))
      if constexpr (KIND == SWAP32_RUN) RUN8("v_permlane32_swap_b32"); else RUN8("v_permlane16_swap_b32");
#undef RUN8
    } else if constexpr (KIND == DPP_QP || KIND == DPP_ROR) {
#pragma unroll
      for (int u = 0; u < 16; u++) {
        if constexpr (KIND == DPP_QP) asm volatile("v_add_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf" : "+v"(a[u]));
        else asm volatile("v_add_f32_dpp %0, %0, %0 row_ror:8 row_mask:0xf bank_mask:0xf" : "+v"(a[u]));
        fma_fill<FM>(f, u, b, c);
      }
    } else {
      // keep = low half (even rows) ? x : y, send = the other; recv = send of lane ^ 32 (^ 16); x = keep + recv
      // Each statement below ends with its exchange still in flight into sd[u], which the compiler does not know: nothing may
      // touch sd[u] between that statement and the s_waitcnt statement behind the loop (nothing does: the fma chains use f[]
      // only, and 66 registers leave no reason to copy or spill).  The kernels keep exchange, wait and add in ONE statement
      // (csrc/bwd_fold.h); here the fma of the interleaved runs have to sit between them.
#pragma unroll
      for (int u = 0; u < 10; u++) {
        if constexpr (KIND == XBAR32)
          asm volatile("v_cndmask_b32_e64 %0, %3, %2, %4\n\tv_cndmask_b32_e64 %1, %2, %3, %4\n\tds_bpermute_b32 %1, %5, %1"
                       : "=&v"(kp[u]), "=&v"(sd[u]) : "v"(a[u]), "v"(y[u]), "s"(m32), "v"(addr));
        else
          asm volatile("v_cndmask_b32_e64 %0, %3, %2, %4\n\tv_cndmask_b32_e64 %1, %2, %3, %4\n\tds_swizzle_b32 %1, %1 offset:swizzle(SWAP,16)"
                       : "=&v"(kp[u]), "=&v"(sd[u]) : "v"(a[u]), "v"(y[u]), "s"(m16));
        fma_fill<FM>(f, u, b, c);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int u = 0; u < 10; u++) asm volatile("v_add_f32 %0, %1, %2" : "=v"(a[u]) : "v"(kp[u]), "v"(sd[u]));
    }
  }
  const unsigned long long t1 = __builtin_amdgcn_s_memtime();
  const unsigned long long r1 = __builtin_amdgcn_s_memrealtime();
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 16; i++) s += a[i] + f[i];
  if (s == 123.456f) sink[0] = s;                      // keeps the chains live; never true
  if ((threadIdx.x & 63) == 0) {
    const size_t w = (size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    stamps[4 * w + 0] = t0; stamps[4 * w + 1] = t1; stamps[4 * w + 2] = r0; stamps[4 * w + 3] = r1;
  }
}

// workgroup shape for k waves per SIMD: min(k, 4) waves per SIMD per workgroup where that divides k, else one wave per SIMD
// per workgroup and k workgroups per CU, held to k by a dynamic LDS size of which k fit into the CU's 160 KiB and k + 1 do not
struct Shape { int threads, wgs_per_cu, lds; };
static Shape shape_for(int k) {
  if (k % std::min(k, 4) == 0) return {256 * std::min(k, 4), k / std::min(k, 4), 0};
  return {256, k, (160 * 1024 / k) / 1024 * 1024};
}

static double g_fma_cycles[16];   // simd cycles per v_fma_f32 at k waves per SIMD (FMA_ONLY runs, from the wall time)

template <int KIND, int FM>
static void run_xchg(const char* name, int k, unsigned long long* d_st, float* d_sink) {
  const Shape sh = shape_for(k);
  const int cus = 256, grid = cus * sh.wgs_per_cu, waves = grid * sh.threads / 64, R = 2048;
  const int units = KIND == FMA_ONLY ? 8 : xchg_units(KIND);
  std::vector<unsigned long long> h(4 * (size_t)waves);
  double best_cyc = 1e30, best_clock = 0, best_ms = 0;
  int occ_blocks = 0;
  hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ_blocks, xchg_kernel<KIND, FM>, sh.threads, sh.lds);
  const int resident = std::min(occ_blocks, sh.wgs_per_cu) * sh.threads / 256;
  for (int rep = 0; rep < 5; rep++) {
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    hipEventRecord(e0);
    hipLaunchKernelGGL((xchg_kernel<KIND, FM>), dim3(grid), dim3(sh.threads), sh.lds, 0, d_st, d_sink, R, 1.0f + rep);
    hipEventRecord(e1); hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1);
    hipMemcpy(h.data(), d_st, h.size() * 8, hipMemcpyDeviceToHost);
    std::vector<double> cyc(waves);
    double clk = 0;
    for (int w = 0; w < waves; w++) {
      cyc[w] = double(h[4 * w + 1] - h[4 * w]) / (double(R) * units);
      clk += double(h[4 * w + 1] - h[4 * w]) / (double(h[4 * w + 3] - h[4 * w + 2]) * 10.0);
    }
    std::sort(cyc.begin(), cyc.end());
    const double med = cyc[waves / 2];
    if (med < best_cyc) { best_cyc = med; best_clock = clk / waves; best_ms = ms; }
    hipEventDestroy(e0); hipEventDestroy(e1);
  }
  // per unit (one exchange and its FM fma): SIMD cycles from the launch's wall time at the measured clock
  const double wall_cyc = best_ms * 1e-3 * best_clock * 1e9;
  const double unit_wall = wall_cyc / (double(waves) * R * units / 1024.0);
  if (KIND == FMA_ONLY) {
    g_fma_cycles[k] = unit_wall / FM;
    printf("{\"instr\": \"v_fma_f32\", \"fma_per_exchange\": %d, \"waves_per_simd_launched\": %d, \"waves_per_simd_resident\": %d, \"workgroup\": %d, "
           "\"grid\": %d, \"simd_cycles_per_fma_from_wall\": %.3f, \"clock_ghz\": %.3f, \"launch_ms\": %.3f}\n",
           FM, k, resident, sh.threads, grid, unit_wall / FM, best_clock, best_ms);
    return;
  }
  printf("{\"instr\": \"%s\", \"fma_per_exchange\": %d, \"waves_per_simd_launched\": %d, \"waves_per_simd_resident\": %d, \"workgroup\": %d, "
         "\"grid\": %d, \"wave_cycles_per_exchange\": %.2f, \"simd_cycles_per_unit_from_wall\": %.2f, "
         "\"simd_cycles_per_exchange_over_fma\": %.2f, \"clock_ghz\": %.3f, \"launch_ms\": %.3f}\n",
         name, FM, k, resident, sh.threads, grid, best_cyc, unit_wall, unit_wall - FM * g_fma_cycles[k], best_clock, best_ms);
  fflush(stdout);
}

template <int KIND>
static void run_kind(const char* name, bool with_fma, unsigned long long* d_st, float* d_sink) {
  for (int k : {1, 2, 4, 5, 7}) run_xchg<KIND, 0>(name, k, d_st, d_sink);
  if constexpr (KIND != SWAP32_RUN && KIND != SWAP16_RUN) {
    if (with_fma)
      for (int k : {1, 5}) { run_xchg<KIND, 8>(name, k, d_st, d_sink); run_xchg<KIND, 16>(name, k, d_st, d_sink); }
  }
}

static int main_xchg(unsigned long long* d_st, float* d_sink) {
  for (int k : {1, 2, 4, 5, 7}) run_xchg<FMA_ONLY, 16>("v_fma_f32", k, d_st, d_sink);
  run_kind<SWAP32>("v_permlane32_swap_b32 (s_nop 1 before and after)", true, d_st, d_sink);
  run_kind<SWAP16>("v_permlane16_swap_b32 (s_nop 1 before and after)", true, d_st, d_sink);
  run_kind<SWAP32_RUN>("v_permlane32_swap_b32 (eight back to back)", false, d_st, d_sink);
  run_kind<SWAP16_RUN>("v_permlane16_swap_b32 (eight back to back)", false, d_st, d_sink);
  run_kind<DPP_QP>("v_add_f32_dpp quad_perm", true, d_st, d_sink);
  run_kind<DPP_ROR>("v_add_f32_dpp row_ror:8", true, d_st, d_sink);
  run_kind<XBAR32>("crossbar lane^32 (2 v_cndmask + ds_bpermute_b32 + v_add_f32)", true, d_st, d_sink);
  run_kind<XBAR16>("crossbar lane^16 (2 v_cndmask + ds_swizzle_b32 + v_add_f32)", true, d_st, d_sink);
  return 0;
}

int main(int argc, char** argv) {
  unsigned long long* d_st; float* d_sink;
  hipMalloc(&d_st, 4 * 8 * (size_t)256 * 32 * 2); hipMalloc(&d_sink, 64);
  if (argc > 1 && !strcmp(argv[1], "xchg")) return main_xchg(d_st, d_sink);
  for (int k : {1, 2, 4, 8}) run<FMA>("v_fma_f32", k, d_st, d_sink);
  for (int k : {1, 2, 4, 8}) run<PKFMA>("v_pk_fma_f32", k, d_st, d_sink);
  for (int k : {1, 2, 4, 8}) run<EXP>("v_exp_f32", k, d_st, d_sink);
  for (int k : {1, 2, 4, 8}) run<MIX>("render_mix", k, d_st, d_sink);
  return 0;
}
