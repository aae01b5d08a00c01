// MV_OP_EXPR columns in the C-PGD tensor-path sweep (pgd.hip constraint_sweep): the value of
// a user-defined column in fp32 and its reverse-mode derivative, lane = row.
//
// mv_pgd_create has checked the bytecode (api.cpp expr_check_tables) and decoded it into one
// int4 per instruction (PgdArgs::xins; the kernels never read the raw words):
//
//   x  opcode (MV_X_*)
//   y  X: feature; K: index into PgdArgs::xk (fp32 constants); SUMF: pool offset o0
//   z  SUMF: pool offset o1
//   w  links: bits 0..7   ordinal of the instruction that produced the left operand (a of a
//                         binary operator, a of WHERE); the right operand (b) is always the
//                         previous instruction, ordinal - 1
//             bits 8..15  WHERE: ordinal of the instruction that produced c
//             bits 16..23 ordinal of the first instruction of this instruction's subtree
//             bit 24      no gradient enters this subtree: the reverse walk pops its adjoint
//                         and continues below the subtree
//
// An instruction's ordinal is its index in the column.  Forward: eight named registers are the
// operand stack (as rowops.h eval_expr: no slot is indexed at run time), and every instruction
// stores its value to the tape, tape[ordinal][row] in the wave's LDS block -- 16 lanes on 16
// banks.  Reverse (only for an active column): the instructions backwards with an adjoint
// stack of eight named registers, starting from 1; an operator pops its adjoint g, reads its
// operands from the tape and pushes their adjoints, the left one first, so the right one is
// on top for the subtree visited next.  The rules are autograd's; a
// zero adjoint is propagated arithmetically (0 / 0 is NaN, as in TF), but the operands of a
// comparison, of AND OR XOR NOT ISNAN ISINF and the condition of WHERE are not part of the
// differentiated graph: their subtrees are stepped over (bit 24).
//
// The tape is the only storage indexed at run time; there is no scratch memory.
#pragma once
#include <hip/hip_runtime.h>

#include "check.h"
#include "pgd.h"

namespace mv {

// np.mod in fp32: the result takes the divisor's sign
__device__ __forceinline__ float xmodf(float a, float b) {
  float m = fmodf(a, b);
  if (m != 0.f) {
    if ((b < 0.f) != (m < 0.f)) m = m + b;
  } else {
    m = copysignf(0.f, b);
  }
  return m;
}

__device__ __forceinline__ float xsgn(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

// The column ins[0 .. n) on the feature-space row XF(f) = (xr[f] - min[f]) / scale[f]; tp is
// this lane's tape column (slot s at tp[s * PGD_ROWS]).
__device__ __forceinline__ float expr_forward(const PgdArgs& a, const int4* __restrict__ ins,
                                              int n, const float* xr, float* tp) {
  const float* __restrict__ sc = a.scale;
  const float* __restrict__ mn = a.minv;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f, s5 = 0.f, s6 = 0.f, s7 = 0.f;
  for (int i = 0; i < n; ++i) {
    const int4 w = ins[i];
    const int op = w.x;
    if (op <= 3) {  // X f, K i, SUMF o0 o1: push
      float v;
      if (op == 1) {
        v = (xr[w.y] - mn[w.y]) / sc[w.y];
      } else if (op == 2) {
        v = a.xk[w.y];
      } else {
        v = 0.f;
        for (int q = w.y; q < w.z; ++q) {
          const int f = a.pool[q];
          v = v + (xr[f] - mn[f]) / sc[f];
        }
      }
      s7 = s6, s6 = s5, s5 = s4, s4 = s3, s3 = s2, s2 = s1, s1 = s0, s0 = v;
    } else if (op <= 20) {  // binary: a . b with b on top
      const float x = s1, y = s0;
      float r;
      switch (op) {
        case 4: r = x + y; break;
        case 5: r = x - y; break;
        case 6: r = x * y; break;
        case 7: r = x / y; break;
        case 8: r = (x < y || x != x) ? x : y; break;  // np.minimum: NaN propagates
        case 9: r = (x > y || x != x) ? x : y; break;  // np.maximum
        case 10: r = xmodf(x, y); break;
        case 11: r = powf(x, y); break;
        case 12: r = x < y ? 1.f : 0.f; break;
        case 13: r = x <= y ? 1.f : 0.f; break;
        case 14: r = x > y ? 1.f : 0.f; break;
        case 15: r = x >= y ? 1.f : 0.f; break;
        case 16: r = x == y ? 1.f : 0.f; break;
        case 17: r = x != y ? 1.f : 0.f; break;
        case 18: r = (x != 0.f) && (y != 0.f) ? 1.f : 0.f; break;
        case 19: r = (x != 0.f) || (y != 0.f) ? 1.f : 0.f; break;
        default: r = (x != 0.f) != (y != 0.f) ? 1.f : 0.f; break;  // 20 XOR
      }
      s0 = r, s1 = s2, s2 = s3, s3 = s4, s4 = s5, s5 = s6, s6 = s7;
    } else if (op <= 26) {  // unary
      const float x = s0;
      switch (op) {
        case 21: s0 = -x; break;
        case 22: s0 = fabsf(x); break;
        case 23: s0 = floorf(x); break;
        case 24: s0 = x == 0.f ? 1.f : 0.f; break;
        case 25: s0 = x != x ? 1.f : 0.f; break;
        default: s0 = fabsf(x) == __builtin_inff() ? 1.f : 0.f; break;  // 26 ISINF
      }
    } else {  // 27 WHERE: c != 0 ? a : b
      s0 = s2 != 0.f ? s1 : s0;
      s1 = s3, s2 = s4, s3 = s5, s4 = s6, s5 = s7;
    }
    tp[MV_IDX(i, a.tape, CK_PGD_TAPE) * PGD_ROWS] = s0;
  }
  return s0;
}

// gr[f] += -(d column / d XF(f)) / scale[f] (the loss is -sum of the columns), from the tape
// expr_forward left.
__device__ __forceinline__ void expr_reverse(const PgdArgs& a, const int4* __restrict__ ins,
                                             int n, float* gr, const float* tp) {
  const float* __restrict__ sc = a.scale;
  float g0 = 1.f, g1 = 0.f, g2 = 0.f, g3 = 0.f, g4 = 0.f, g5 = 0.f, g6 = 0.f, g7 = 0.f;
  for (int i = n - 1; i >= 0; --i) {
    const int4 w = ins[i];
    const int op = w.x;
    const float g = g0;
    if ((w.w >> 24) & 1) {  // outside the differentiated graph: drop g, step over the subtree
      g0 = g1, g1 = g2, g2 = g3, g3 = g4, g4 = g5, g5 = g6, g6 = g7;
      i = (w.w >> 16) & 0xFF;
      continue;
    }
    if (op <= 3) {  // leaf: pop
      g0 = g1, g1 = g2, g2 = g3, g3 = g4, g4 = g5, g5 = g6, g6 = g7;
      if (op == 1) {
        gr[w.y] = gr[w.y] + (-g) / sc[w.y];
      } else if (op == 3) {
        for (int q = w.y; q < w.z; ++q) {
          const int f = a.pool[q];
          gr[f] = gr[f] + (-g) / sc[f];
        }
      }
    } else if (op <= 11) {  // differentiable binary: g -> (ga, gb), gb on top
      const float x = tp[MV_IDX(w.w & 0xFF, a.tape, CK_PGD_TAPE) * PGD_ROWS];
      const float y = tp[MV_IDX(i - 1, a.tape, CK_PGD_TAPE) * PGD_ROWS];
      float ga, gb;
      switch (op) {
        case 4: ga = g; gb = g; break;
        case 5: ga = g; gb = -g; break;
        case 6: ga = g * y; gb = g * x; break;
        case 7: ga = g / y; gb = -(g * x) / (y * y); break;
        case 8: ga = y < x ? 0.f : g; gb = y < x ? g : 0.f; break;  // first on a tie
        case 9: ga = y > x ? 0.f : g; gb = y > x ? g : 0.f; break;
        case 10: ga = g; gb = -g * floorf(x / y); break;
        default: {  // 11 POW
          const float q = tp[MV_IDX(i, a.tape, CK_PGD_TAPE) * PGD_ROWS];
          ga = g * (y * powf(x, y - 1.f));
          gb = (x == 0.f && y >= 0.f) ? 0.f : g * (q * logf(x));
        } break;
      }
      g7 = g6, g6 = g5, g5 = g4, g4 = g3, g3 = g2, g2 = g1, g1 = ga, g0 = gb;
    } else if (op <= 26) {  // unary (NOT ISNAN ISINF are stepped over above)
      const float x = tp[MV_IDX(i - 1, a.tape, CK_PGD_TAPE) * PGD_ROWS];
      g0 = op == 21 ? -g : (op == 22 ? g * xsgn(x) : 0.f);  // NEG, ABS, FLOOR
    } else {  // 27 WHERE (c, a, b): c is stepped over when the walk reaches it
      const float c = tp[MV_IDX((w.w >> 8) & 0xFF, a.tape, CK_PGD_TAPE) * PGD_ROWS];
      const float ga = c != 0.f ? g : 0.f, gb = c != 0.f ? 0.f : g;
      g7 = g5, g6 = g4, g5 = g3, g4 = g2, g3 = g1, g2 = 0.f, g1 = ga, g0 = gb;
    }
  }
}

}  // namespace mv
