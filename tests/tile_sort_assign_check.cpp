// Stand-alone check of gaussianip_amd/csrc/tile_sort_assign.h (built and run by test_tile_sort_assign_cpu.py with the host
// compiler and -fsanitize=address,undefined).  For every grid size and every triple of class counts it walks the static round
// exactly as gip_tile_sort_kernel does and asserts:
//   * every position of [0, end_b) is claimed once: by one (workgroup), one (workgroup, quarter), one (workgroup, wave), or by
//     lying in the range left to one of the two cursors; nothing is claimed twice, nothing outside its class;
//   * no workgroup with a first-round A tile holds a static M tile; nobody holds more than four quarters;
//   * the cursor offsets equal what the static round covered, and the M cursor is used only when the M tiles outnumber the
//     free workgroups by more than four to one;
//   * B goes to the least loaded first, by tier (no M quarter | one to three | four | an A tile): a workgroup gets a
//     first-round B tile only if every wave of every workgroup of a lower tier has one, and inside a tier the first-round
//     counts differ by at most one.
// Prints "ok <cases>" and exits 0, or the first violation and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "tile_sort_assign.h"

static long g_cases = 0;

#define CHECK(cond, what)                                                                                            \
  do {                                                                                                               \
    if (!(cond)) {                                                                                                   \
      std::printf("FAIL grid %u A %u M %u B %u: %s (%s)\n", grid, na, nm, nb, what, #cond);                           \
      std::exit(1);                                                                                                  \
    }                                                                                                                \
  } while (0)

static void check(uint32_t grid, uint32_t na, uint32_t nm, uint32_t nb, std::vector<uint8_t>& claimed) {
  const uint32_t end_a = na, end_m = na + nm, end_b = na + nm + nb;
  const GipSortAssign s = gip_sort_assign(grid, end_a, end_m, end_b);
  claimed.assign(end_b, 0);
  g_cases++;
  // class A
  uint32_t a_static = 0;
  for (uint32_t wg = 0; wg < grid; wg++) {
    const uint32_t p = gip_sort_a_pos(s, wg);
    CHECK(p <= end_a, "A position outside the class");
    if (p < end_a) { claimed[p]++; a_static++; }
  }
  CHECK(s.a_first == a_static, "A cursor offset is not what the static round covered");
  CHECK(a_static == (na < grid ? na : grid), "the static A round is not min(A, grid)");
  for (uint32_t p = s.a_first; p < end_a; p++) claimed[p]++;
  // class M
  uint32_t m_static = 0;
  const uint32_t free_wgs = grid - a_static;
  for (uint32_t wg = 0; wg < grid; wg++) {
    const uint32_t mq = gip_sort_m_quarters(s, wg);
    CHECK(mq <= GIP_SORT_QUARTERS, "more than four quarters");
    if (gip_sort_a_pos(s, wg) < end_a) CHECK(mq == 0, "an A holder got a static M tile");
    for (uint32_t q = 0; q < mq; q++) {
      const uint32_t p = gip_sort_m_pos(s, wg, q);
      CHECK(p >= end_a && p < end_m, "M position outside the class");
      claimed[p]++;
      m_static++;
    }
    if ((uint64_t)nm > 4ull * free_wgs && gip_sort_a_pos(s, wg) >= end_a) CHECK(mq == GIP_SORT_QUARTERS, "M outnumbers the free workgroups: four each");
  }
  CHECK(s.m_drawn == end_a + m_static, "M cursor offset is not what the static round covered");
  CHECK(s.m_drawn <= end_m, "M cursor offset beyond the class");
  if ((uint64_t)nm <= 4ull * free_wgs) CHECK(s.m_drawn == end_m, "M fits four per free workgroup but is drawn");
  for (uint32_t p = s.m_drawn; p < end_m; p++) claimed[p]++;
  // class B
  const uint32_t stride = gip_sort_b_stride(s);
  CHECK(stride == grid * GIP_SORT_WAVES, "B stride");
  // first-round B tiles per workgroup, by load: [0] = smallest count among the workgroups of that load, [1] = largest
  uint32_t lo[4], hi[4];
  for (int k = 0; k < 4; k++) { lo[k] = ~0u; hi[k] = 0; }
  for (uint32_t wg = 0; wg < grid; wg++) {
    uint32_t first = 0;
    for (uint32_t w = 0; w < GIP_SORT_WAVES; w++) {
      uint32_t p = gip_sort_b_pos(s, wg, w);
      CHECK(p >= end_m, "B position in front of the class");
      if (p < end_b) first++;
      for (; p < end_b; p += stride) claimed[p]++;
    }
    const uint32_t mq = gip_sort_m_quarters(s, wg);
    const int load = gip_sort_a_pos(s, wg) < end_a ? 3 : mq == 0 ? 0 : mq < GIP_SORT_QUARTERS ? 1 : 2;
    if (first < lo[load]) lo[load] = first;
    if (first > hi[load]) hi[load] = first;
  }
  for (int a = 0; a < 4; a++) {
    if (lo[a] != ~0u) CHECK(hi[a] - lo[a] <= 1, "B is not dealt evenly inside a tier");
    for (int b = a + 1; b < 4; b++)
      if (lo[a] != ~0u && lo[b] != ~0u && hi[b] > 0) CHECK(lo[a] == GIP_SORT_WAVES, "a heavier workgroup got a B tile before a lighter one was full");
  }
  for (uint32_t p = 0; p < end_b; p++) CHECK(claimed[p] == 1, claimed[p] ? "a position is claimed twice" : "a position is not claimed");
}

int main() {
  const uint32_t grids[] = {1, 2, 8, 255, 256, 304};
  std::vector<uint8_t> claimed;
  for (uint32_t grid : grids) {
    const uint32_t top = 3 * grid + 5;
    if (grid <= 8) {                       // the whole cube
      for (uint32_t na = 0; na <= top; na++)
        for (uint32_t nm = 0; nm <= top; nm++)
          for (uint32_t nb = 0; nb <= top; nb++) check(grid, na, nm, nb, claimed);
    } else {
      // every count of one class against the edges of the other two (an empty class, one tile, one per workgroup, between two
      // and three rounds, the top)
      const uint32_t edge[] = {0, 1, grid, 2 * grid + 3, top};
      for (uint32_t full = 0; full <= top; full++)
        for (uint32_t e1 : edge)
          for (uint32_t e2 : edge) {
            check(grid, full, e1, e2, claimed);
            check(grid, e1, full, e2, claimed);
            check(grid, e1, e2, full, claimed);
          }
    }
    // M beyond four per workgroup (the drawn rounds) and B beyond two rounds of wave slots, with and without A holders
    const uint32_t as[] = {0, 1, grid / 2, grid - 1, grid, grid + 7};
    const uint32_t ms[] = {4 * grid - 1, 4 * grid, 4 * grid + 1, 5 * grid + 3, 9 * grid};
    const uint32_t bs[] = {0, 16 * grid - 1, 16 * grid, 16 * grid + 1, 33 * grid + 5};
    for (uint32_t na : as)
      for (uint32_t nm : ms)
        for (uint32_t nb : bs) check(grid, na, nm, nb, claimed);
    for (uint32_t na : as)
      for (uint32_t nb : bs) check(grid, na, 3, nb, claimed);
  }
  std::printf("ok %ld\n", g_cases);
  return 0;
}
