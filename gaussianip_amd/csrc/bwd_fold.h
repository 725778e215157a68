// bwd_fold.h — the cross-lane fold of the backward blend (render_backward.hip): TWO list entries' ten terms at once,
// 20 accumulators of 64 lanes -> 20 sums.  Two networks with the same summation trees and the same result lanes:
//   fold_two_entries       the one the library launches: levels 32 and 16 exchange half-waves over the LDS crossbar
//                          (ds_bpermute_b32 / ds_swizzle_b32: no LDS allocated, no vector issue slot for the move)
//   fold_two_entries_swap  the v_permlane32/16_swap network it replaces; launched by nothing in the library, kept for the
//                          bit-equality check and the micro A/B (tools/micro/fold_check.hip)
//
// Every sum keeps the summation tree of the one-entry fold both descend from, so the rows are bit-identical to its rows:
//     terms 0-7   T(q), q[i] = (x[i] + x[i+32]) + (x[i+16] + x[i+48]),
//     terms 8, 9  T(h[16..31]) + T(h[0..15]), h[i] = x[i] + x[i+32],
// with T the 16-lane tree over neighbours, pairs of neighbours, quads and halves (float addition commutes, so only the
// pairing matters, not which lane holds a sum nor which operand travelled).  What the fold costs is its DPP and swap
// instructions, not its instruction count (profiles/bwd_pair_fold.txt, profiles/lane_exchange_rate.txt), so the network
// spends plain selects to halve the registers BEFORE each DPP level:
//   level 32  a_t + b_t with entry A's half sums in lanes 0-31 and entry B's in lanes 32-63
//             swap:      v_permlane32_swap(a_t, b_t): a_t = [a_lo | b_lo], b_t = [a_hi | b_hi]         10 swaps + 10 adds
//             crossbar:  keep = lane < 32 ? a_t : b_t, send = the other, recv = send of lane ^ 32 (ds_bpermute), keep + recv:
//                        lanes 0-31 a_t[i] + a_t[i+32], lanes 32-63 b_t[i] + b_t[i-32], the swap network's operand pairs
//                                                                                   20 selects + 10 bpermutes + 10 adds
//   level 16  on the term pairs (x, y) = (0,1) (2,3) (4,5) (6,7): rows [x_r0+x_r1, y_r0+y_r1, x_r2+x_r3, y_r2+y_r3], i.e.
//             [A_t, A_t+1, B_t, B_t+1]; on (8,9) the exchange alone: x = first rows [A_8, A_9, B_8, B_9] of the half sums,
//             y = their second rows
//             swap:      v_permlane16_swap (odd rows of x <-> even rows of y), then x + y                 5 swaps +  4 adds
//             crossbar:  keep = even row ? x : y, send = the other, recv = send of lane ^ 16 (ds_swizzle SWAP,16), keep + recv;
//                        on (8,9) x = even row ? x : recv, y = even row ? recv : y            11 selects + 5 swizzles + 4 adds
//   level 1   per register pair (x, y): u = even lanes of x | odd lanes of y, v = the other lanes; quad_perm:[1,0,3,2](v) + u
//             holds x's neighbour sums in the even lanes and y's in the odd ones: 6 -> 3 registers   6 selects + 3 DPP adds
//   level 2   the same on bit 1 of the lane with quad_perm:[2,3,0,1]: 3 -> 2 registers              2 selects + 2 DPP adds
//   level 4   bank-masked DPP adds (banks 0, 2 with row_shl:4, banks 1, 3 from the other register with row_shr:4; the
//             unwritten banks keep the destination): 2 -> 1 register                                2 DPP adds
//   level 8   row_ror:8                                                                             1 DPP add
//   terms 8, 9: odd lane (second row's tree) + even lane (first row's), banks 1, 3 only             1 DPP add
// Result: b8, lanes 16 r + j (j = 0..3): entry r >> 1, term 2 j + (r & 1); lanes 16 r + 4: entry r >> 1, term 8 + (r & 1).
// Entry A's term t and entry B's term t go through the SAME tree (the same lanes of another row at every level), so an
// entry's row does not depend on its slot in the pair nor on its partner.
// One asm statement per network: the compiler pads no hazard inside one, so the order below keeps at least two wait states
// between every vector write and the v_permlane / DPP read of that register (s_nop where no independent work is left), and
// the crossbar exchanges carry their own s_waitcnt (all exchanges of a level are issued back to back, the LDS returns them
// in order).  Inline asm for the swaps because the clang builtin mis-selects its second result for float operands on
// ROCm 7.2 (both extracts return the first register); the whole wave must be active (wave-uniform control flow only: an
// inactive lane would hand its partner a zero).
#pragma once
#include <stdint.h>

struct BwdAcc { float v0, v1, v2, v3, v4, v5, v6, v7, v8, v9; };

#define GIP_DPP(d, s, ctrl, bank) "v_add_f32_dpp " d ", " s ", " s " " ctrl " row_mask:0xf bank_mask:" bank "\n\t"
#define GIP_QP1 "quad_perm:[1,0,3,2]"
#define GIP_QP2 "quad_perm:[2,3,0,1]"
// levels 1, 2, 4, 8 and the terms-8/9 add, shared by both networks: in %0 %2 %4 %6 (terms 0-7) %8 %9, scratch %10-%18,
// out %18; EVEN / BIT1 name the operands that hold the lane masks 0xaaaa... and 0xcccc...
#define GIP_FOLD_ROWS(EVEN, BIT1)                                                                                            \
      /* level 1, two registers per DPP add: u = even lanes of x | odd lanes of y, v = the other lanes; dpp(v) + u leaves */ \
      /* x's neighbour sums in the even lanes and y's in the odd ones   %10 <- %0 | %2   %12 <- %4 | %6   %14 <- %8 | %9  */ \
      "v_cndmask_b32_e64 %10, %0, %2, " EVEN "\n\tv_cndmask_b32_e64 %11, %2, %0, " EVEN "\n\t"                               \
      "v_cndmask_b32_e64 %12, %4, %6, " EVEN "\n\tv_cndmask_b32_e64 %13, %6, %4, " EVEN "\n\t"                               \
      "v_cndmask_b32_e64 %14, %8, %9, " EVEN "\n\tv_cndmask_b32_e64 %15, %9, %8, " EVEN "\n\t"                               \
      "v_add_f32_dpp %10, %11, %10 " GIP_QP1 " row_mask:0xf bank_mask:0xf\n\t"                                               \
      "v_add_f32_dpp %12, %13, %12 " GIP_QP1 " row_mask:0xf bank_mask:0xf\n\t"                                               \
      "v_add_f32_dpp %14, %15, %14 " GIP_QP1 " row_mask:0xf bank_mask:0xf\n\t"                                               \
      /* level 2, the same on bit 1 of the lane: %16 <- %10 (lanes 0, 1 of a quad) | %12 (lanes 2, 3); %14 on its own */     \
      "v_cndmask_b32_e64 %17, %12, %10, " BIT1 "\n\tv_cndmask_b32_e64 %16, %10, %12, " BIT1 "\n\t"                           \
      "v_add_f32_dpp %14, %14, %14 " GIP_QP2 " row_mask:0xf bank_mask:0xf\n\t"                                               \
      "v_add_f32_dpp %16, %17, %16 " GIP_QP2 " row_mask:0xf bank_mask:0xf\n\t"                                               \
      "s_nop 0\n\t"                                                                                                          \
      /* level 4: banks 0, 2 <- %16, banks 1, 3 <- %14;  level 8;  terms 8, 9: odd lane (second row's tree) + even lane */   \
      GIP_DPP("%18", "%14", "row_shr:4", "0xa") GIP_DPP("%18", "%16", "row_shl:4", "0x5")                                    \
      "s_nop 1\n\t"                                                                                                          \
      GIP_DPP("%18", "%18", "row_ror:8", "0xf")                                                                              \
      "s_nop 1\n\t"                                                                                                          \
      "v_add_f32_dpp %18, %18, %18 " GIP_QP1 " row_mask:0xf bank_mask:0xa"

// level 32 of terms %0-%9 (entry A) and %10-%19 (entry B) by swaps: sums in %0-%9, %10-%19 free
#define GIP_FOLD_L32_SWAP                                                                                                    \
      "s_nop 1\n\t"                                                                                                          \
      "v_permlane32_swap_b32 %0, %10\n\tv_permlane32_swap_b32 %1, %11\n\tv_permlane32_swap_b32 %2, %12\n\t"                  \
      "v_permlane32_swap_b32 %3, %13\n\tv_permlane32_swap_b32 %4, %14\n\tv_permlane32_swap_b32 %5, %15\n\t"                  \
      "v_permlane32_swap_b32 %6, %16\n\tv_permlane32_swap_b32 %7, %17\n\tv_permlane32_swap_b32 %8, %18\n\t"                  \
      "v_permlane32_swap_b32 %9, %19\n\t"                                                                                    \
      "v_add_f32 %0, %0, %10\n\tv_add_f32 %1, %1, %11\n\tv_add_f32 %2, %2, %12\n\tv_add_f32 %3, %3, %13\n\t"                 \
      "v_add_f32 %4, %4, %14\n\tv_add_f32 %5, %5, %15\n\tv_add_f32 %6, %6, %16\n\tv_add_f32 %7, %7, %17\n\t"                 \
      "v_add_f32 %8, %8, %18\n\tv_add_f32 %9, %9, %19\n\t"
// level 16 of %0-%9 by swaps: sums of the term pairs in %0 %2 %4 %6, the exchanged (8,9) in %8 %9
#define GIP_FOLD_L16_SWAP                                                                                                    \
      "v_permlane16_swap_b32 %0, %1\n\tv_permlane16_swap_b32 %2, %3\n\tv_permlane16_swap_b32 %4, %5\n\t"                     \
      "v_permlane16_swap_b32 %6, %7\n\tv_permlane16_swap_b32 %8, %9\n\t"                                                     \
      "v_add_f32 %0, %0, %1\n\tv_add_f32 %2, %2, %3\n\tv_add_f32 %4, %4, %5\n\tv_add_f32 %6, %6, %7\n\t"
// one level-16 exchange over the crossbar: K <- keep = even row ? X : Y;  S <- send = even row ? Y : X;  S <- S of lane ^ 16
#define GIP_X16(X, Y, K, S, ROWS)                                                                                            \
      "v_cndmask_b32_e64 " K ", " Y ", " X ", " ROWS "\n\tv_cndmask_b32_e64 " S ", " X ", " Y ", " ROWS "\n\t"               \
      "ds_swizzle_b32 " S ", " S " offset:swizzle(SWAP,16)\n\t"
// the end of level 16 over the crossbar, after the exchanges of (0,1) (2,3) (4,5) (6,7) into (%10,%11) ... (%16,%17): the (8,9)
// exchange through %18, the wait, the four adds and the two selects of (8,9).  Same outputs as GIP_FOLD_L16_SWAP
#define GIP_FOLD_L16_XBAR_END(ROWS)                                                                                          \
      "v_cndmask_b32_e64 %18, %8, %9, " ROWS "\n\tds_swizzle_b32 %18, %18 offset:swizzle(SWAP,16)\n\t"                       \
      "s_waitcnt lgkmcnt(0)\n\t"                                                                                             \
      "v_add_f32 %0, %10, %11\n\tv_add_f32 %2, %12, %13\n\tv_add_f32 %4, %14, %15\n\tv_add_f32 %6, %16, %17\n\t"             \
      "v_cndmask_b32_e64 %8, %18, %8, " ROWS "\n\tv_cndmask_b32_e64 %9, %9, %18, " ROWS "\n\t"

#define GIP_FOLD_ACCS                                                                                                        \
      "+v"(a.v0), "+v"(a.v1), "+v"(a.v2), "+v"(a.v3), "+v"(a.v4), "+v"(a.v5), "+v"(a.v6), "+v"(a.v7), "+v"(a.v8), "+v"(a.v9), \
      "+v"(b.v0), "+v"(b.v1), "+v"(b.v2), "+v"(b.v3), "+v"(b.v4), "+v"(b.v5), "+v"(b.v6), "+v"(b.v7), "+v"(b.v8), "+v"(b.v9)

// the swap network (check and micro A/B only): 15 swaps, 9 DPP adds, 14 plain adds and 8 selects
__device__ __forceinline__ void fold_two_entries_swap(BwdAcc& a, BwdAcc& b) {
  asm volatile(GIP_FOLD_L32_SWAP GIP_FOLD_L16_SWAP GIP_FOLD_ROWS("%20", "%21")
               : GIP_FOLD_ACCS
               : "s"(0xaaaaaaaaaaaaaaaaull), "s"(0xccccccccccccccccull));
}

// the launched network, both levels over the crossbar: 10 bpermutes, 5 swizzles, 9 DPP adds, 14 plain adds and 39 selects.
// xaddr = (lane ^ 32) << 2, the bpermute's byte address.  Level 32 keeps in place and sends from a rotating free register
// (%20, then each b_t as its term has been split), so the exchange costs one register beyond the twenty accumulators; its
// adds and the first exchanges of level 16 start as soon as the bpermutes they need have returned (lgkmcnt counts down in
// issue order).
__device__ __forceinline__ void fold_two_entries(BwdAcc& a, BwdAcc& b, int xaddr) {
  float x;
#define GIP_X32(A, B, S) /* S <- send = lane < 32 ? B : A;  A <- keep = lane < 32 ? A : B;  S <- S of lane ^ 32 */ \
  "v_cndmask_b32_e64 " S ", " A ", " B ", %22\n\tv_cndmask_b32_e64 " A ", " B ", " A ", %22\n\tds_bpermute_b32 " S ", %21, " S "\n\t"
  asm volatile(
      GIP_X32("%0", "%10", "%20") GIP_X32("%1", "%11", "%10") GIP_X32("%2", "%12", "%11") GIP_X32("%3", "%13", "%12")
      GIP_X32("%4", "%14", "%13") GIP_X32("%5", "%15", "%14") GIP_X32("%6", "%16", "%15") GIP_X32("%7", "%17", "%16")
      GIP_X32("%8", "%18", "%17") GIP_X32("%9", "%19", "%18")
      "s_waitcnt lgkmcnt(6)\n\t"
      "v_add_f32 %0, %0, %20\n\tv_add_f32 %1, %1, %10\n\tv_add_f32 %2, %2, %11\n\tv_add_f32 %3, %3, %12\n\t"
      "s_waitcnt lgkmcnt(2)\n\t"
      "v_add_f32 %4, %4, %13\n\tv_add_f32 %5, %5, %14\n\tv_add_f32 %6, %6, %15\n\tv_add_f32 %7, %7, %16\n\t"
      GIP_X16("%0", "%1", "%10", "%11", "%23") GIP_X16("%2", "%3", "%12", "%13", "%23")
      "s_waitcnt lgkmcnt(2)\n\t"
      "v_add_f32 %8, %8, %17\n\tv_add_f32 %9, %9, %18\n\t"
      GIP_X16("%4", "%5", "%14", "%15", "%23") GIP_X16("%6", "%7", "%16", "%17", "%23")
      GIP_FOLD_L16_XBAR_END("%23") GIP_FOLD_ROWS("%24", "%25")
      : GIP_FOLD_ACCS, "=&v"(x)
      : "v"(xaddr), "s"(0x00000000ffffffffull), "s"(0x0000ffff0000ffffull), "s"(0xaaaaaaaaaaaaaaaaull),
        "s"(0xccccccccccccccccull));
#undef GIP_X32
}

#undef GIP_FOLD_ACCS
#undef GIP_FOLD_L32_SWAP
#undef GIP_FOLD_L16_SWAP
#undef GIP_FOLD_L16_XBAR_END
#undef GIP_X16
#undef GIP_FOLD_ROWS
#undef GIP_DPP
#undef GIP_QP1
#undef GIP_QP2
