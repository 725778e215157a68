// tile_sort_assign.h — who sorts which tile in gip_tile_sort_kernel's first round (binning.hip).
//
// tile_order lists the tiles longest class first: A = [0, end_a) (lists >= 2048 entries, one workgroup each), M = [end_a, end_m)
// (512..2047, one 256-thread quarter each), B = [end_m, end_b) (1..511, one wave each).  Every workgroup computes its share from
// these three numbers, the grid size and its own index: no counter, no round trip.
//   A  position wg if wg < end_a.  What is left, [grid, end_a), is drawn from GipRasterHeader::sort_cursor.
//   M  dealt to the `free` workgroups, those without a first-round A tile, one position per (round k, free index f):
//      end_a + k * free + f.  Rounds = ceil(n_M / free), at most 4 (the four quarters of one pass of the workgroup); what four
//      rounds do not cover, [m_drawn, end_m), is drawn from sort_cursor_m four at a time.  A free workgroup holds m_base or
//      m_base + 1 quarters; the first m_rem of them hold the larger number.
//   B  one position per wave slot; the grid has 16 * grid slots per round.  The slots are numbered so that the least loaded
//      workgroups are filled first, by tier: all waves of the free workgroups without an M quarter, then of those with one to
//      three, then of those with four, then of the A holders.  (A 512-key network costs a CU the same in a B tile as in an M
//      quarter: measured, sixteen of the longest B tiles on one workgroup take longer than two M quarters and ten B tiles, so
//      the tiers are no finer than that.)  The free workgroups fall into at most two tiers, "light" and "heavy".  Inside a
//      tier consecutive slots — consecutive positions, lists of similar length — lie on different workgroups (slot = wave *
//      tier size + index in tier).  Positions beyond one round of slots wrap around: slot s sorts end_m + s, end_m + s + 16 *
//      grid, ...
// Plain C++ (host and device): the CPU test includes it as it is.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GIP_ASSIGN_FN __host__ __device__ inline
#else
#define GIP_ASSIGN_FN inline
#endif

#define GIP_SORT_WAVES 16u          // waves of a tile-sort workgroup (1024 threads)
#define GIP_SORT_QUARTERS 4u        // 256-thread quarters of it: M tiles of one pass

struct GipSortAssign {
  uint32_t grid, end_a, end_m, end_b;
  uint32_t a_first;      // workgroups holding a first-round A tile = min(end_a, grid); sort_cursor draws start at position a_first
  uint32_t free;         // workgroups without one
  uint32_t m_static;     // M positions the static round covers
  uint32_t m_base, m_rem;// a free workgroup f holds m_base + (f < m_rem) quarters
  uint32_t m_drawn;      // sort_cursor_m draws start at this position (== end_m: nothing is drawn)
  uint32_t b_heavy;      // free workgroups [0, b_heavy) are a tier above the others for B (0: one tier)
};

GIP_ASSIGN_FN GipSortAssign gip_sort_assign(uint32_t grid, uint32_t end_a, uint32_t end_m, uint32_t end_b) {
  GipSortAssign s;
  s.grid = grid; s.end_a = end_a; s.end_m = end_m; s.end_b = end_b;
  s.a_first = end_a < grid ? end_a : grid;
  s.free = grid - s.a_first;
  const uint32_t n_m = end_m - end_a;
  const uint32_t cap = s.free * GIP_SORT_QUARTERS;        // grid <= a few hundred: no overflow
  s.m_static = n_m < cap ? n_m : cap;
  s.m_base = s.free ? s.m_static / s.free : 0u;
  s.m_rem = s.free ? s.m_static % s.free : 0u;
  s.m_drawn = end_a + s.m_static;
  // quarters m_base and m_base + 1 lie in different tiers (0 | 1..3 | 4) only across 0 -> 1 and 3 -> 4
  s.b_heavy = (s.m_base == 0u || s.m_base == 3u) ? s.m_rem : 0u;
  return s;
}

// first-round A position of workgroup wg, or end_a if it has none
GIP_ASSIGN_FN uint32_t gip_sort_a_pos(const GipSortAssign& s, uint32_t wg) { return wg < s.a_first ? wg : s.end_a; }

// M quarters workgroup wg holds in the static round (0 .. 4); quarter q < that number sorts position gip_sort_m_pos(s, wg, q)
GIP_ASSIGN_FN uint32_t gip_sort_m_quarters(const GipSortAssign& s, uint32_t wg) {
  if (wg < s.a_first) return 0u;
  return s.m_base + ((wg - s.a_first) < s.m_rem ? 1u : 0u);
}
GIP_ASSIGN_FN uint32_t gip_sort_m_pos(const GipSortAssign& s, uint32_t wg, uint32_t q) { return s.end_a + q * s.free + (wg - s.a_first); }

// first B position of (workgroup wg, wave wave); the wave goes on in steps of gip_sort_b_stride while the position is below end_b.
// A workgroup's waves are filled from the last one down: M quarters are dealt from the first one up, and a wave whose quarter
// holds no M tile sorts its B tiles while the other quarters are in their register networks.
GIP_ASSIGN_FN uint32_t gip_sort_b_pos(const GipSortAssign& s, uint32_t wg, uint32_t wave) {
  const uint32_t w = GIP_SORT_WAVES - 1u - wave;
  const uint32_t heavy = s.b_heavy, light = s.free - s.b_heavy;   // free workgroups [a_first, a_first + heavy) are the heavy ones
  uint32_t slot;
  if (wg < s.a_first) slot = s.free * GIP_SORT_WAVES + w * s.a_first + wg;
  else if (wg - s.a_first < heavy) slot = light * GIP_SORT_WAVES + w * heavy + (wg - s.a_first);
  else slot = w * light + (wg - s.a_first - heavy);
  return s.end_m + slot;
}
GIP_ASSIGN_FN uint32_t gip_sort_b_stride(const GipSortAssign& s) { return s.grid * GIP_SORT_WAVES; }
