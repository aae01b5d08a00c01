// C-PGD on device: the whole gradient attack of src/attacks/pgd/atk.py:74-163 (ART's
// ProjectedGradientDescentTensorFlowV2 loop) + src/attacks/pgd/classifier.py:107-332
// (loss_gradient) in one launch.  Every row is independent: a wave owns a tile of 16 rows and
// runs, max_iter times, forward MLP, backward MLP, the tensor-path constraint columns and
// their reverse sweep, then mask / normalise / step / clip / project / repair.  Dense layers
// run on v_mfma_f32_16x16x4f32 (forward A.W, backward dZ.W^T with the ReLU masks read from
// the kept activations); the last (softmax) layer has <= 8 columns and runs on the VALU.
//
// LDS per workgroup: the weights (row stride N + 1, so the forward read W[k][col] and the
// transposed backward read W[col][k] are both conflict free), staged once; per wave the x
// tile, the gradient tile, the hidden activations and two dZ buffers.  A first layer too
// large for LDS (botnet: 756 x 64) is streamed from L2.
//
// fp32 throughout, built with -ffp-contract=off: the per-row arithmetic is the order written
// in DESIGN.md section 7a, which tests/pgd_torch_ref.py restates.
//
// k_pgd<true> / k_pgd_grad<true> are the instances for a tensor program with MV_OP_EXPR
// columns (pgd_expr.h: an fp32 interpreter with a value tape in LDS and a reverse sweep); a
// program without one runs the <false> instances, which hold no interpreter code.
#include <hip/hip_runtime.h>

#include "../../include/moeva_mi355x.h"
#include "pgd.h"
#include "pgd_expr.h"
#include "wave.h"

namespace mv {

typedef float pgd_f4 __attribute__((ext_vector_type(4)));

namespace {

// Per-wave LDS tile (pointers into the dynamic LDS block).
struct PgdTile {
  float* xs;                      // [16][Dp] current scaled rows
  float* gs;                      // [16][Dp] gradient, then the projected perturbation
  float* h[PGD_MAX_LAYERS];       // h[l]: [16][dims[l] + 1] post-ReLU activations, l >= 1
  float* dz[2];                   // [16][hmax + 1]
  float* dl;                      // [16][PGD_MAX_OUT] d loss / d logit
  float* lossc;                   // [16] cross-entropy
  int* ys;                        // [16] labels; EXPR instances: then the value tape
                                  // [a.tape][16] of one EXPR column (pgd_tape)
  const float* W[PGD_MAX_LAYERS]; // LDS (staged) or global
  int ldw[PGD_MAX_LAYERS];
};

__device__ __forceinline__ int pgd_hmax(const PgdArgs& a) {
  int m = 16;
  for (int l = 1; l < a.n_layers; ++l) m = a.dims[l] > m ? a.dims[l] : m;
  return m;
}

__device__ __forceinline__ float sgn(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

// out[16][N] = relu(in[16][K] . W[K][N] + bias), N % 16 == 0.  A operand lane (il, ka) holds
// in[il][k0 + ka], B operand W[k0 + ka][col tile + il]; acc[j] is row ka * 4 + j, column il.
__device__ __forceinline__ void dense_fwd(const float* in, int ldi, int K, const float* W,
                                          int ldw, const float* __restrict__ bias, int N,
                                          float* out, int ldo, int lane) {
  const int ka = lane >> 4, il = lane & 15;
  const int nct = N >> 4;
  for (int c0 = 0; c0 < nct; c0 += 4) {
    pgd_f4 acc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = pgd_f4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < K; k0 += 4) {
      const int k = k0 + ka;
      const bool ok = k < K;
      const float av = ok ? in[il * ldi + k] : 0.f;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (c0 + c < nct) {
          const float bv = ok ? W[(size_t)k * ldw + (c0 + c) * 16 + il] : 0.f;
          acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[c], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (c0 + c < nct) {
        const int col = (c0 + c) * 16 + il;
        const float bv = bias[col];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float v = acc[c][j] + bv;
          out[(ka * 4 + j) * ldo + col] = v > 0.f ? v : 0.f;
        }
      }
    }
  }
}

// din[16][K] = dz[16][N] . W^T (W [K][N]), N % 16 == 0; with hprev the ReLU mask of the layer
// below (relu'(0) = 0).  B operand lane (il, ka) holds W[col tile + il][n0 + ka].
__device__ __forceinline__ void dense_bwd(const float* dz, int ldz, int N, const float* W,
                                          int ldw, int K, const float* hprev, int ldh,
                                          float* din, int ldd, int lane) {
  const int ka = lane >> 4, il = lane & 15;
  const int nct = (K + 15) >> 4;
  for (int c0 = 0; c0 < nct; c0 += 4) {
    pgd_f4 acc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = pgd_f4{0.f, 0.f, 0.f, 0.f};
    for (int n0 = 0; n0 < N; n0 += 4) {
      const float av = dz[il * ldz + n0 + ka];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (c0 + c < nct) {
          const int col = (c0 + c) * 16 + il;
          const float bv = col < K ? W[(size_t)col * ldw + n0 + ka] : 0.f;
          acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[c], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int col = (c0 + c) * 16 + il;
      if (c0 + c < nct && col < K) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int row = ka * 4 + j;
          float v = acc[c][j];
          if (hprev) v = hprev[row * ldh + col] > 0.f ? v : 0.f;
          din[row * ldd + col] = v;
        }
      }
    }
  }
}

// Hidden layers forward: t.xs -> t.h[1 .. L-1].
__device__ __forceinline__ void mlp_forward(const PgdArgs& a, const PgdTile& t, int lane) {
  const int L = a.n_layers;
  for (int l = 0; l < L - 1; ++l) {
    const float* in = l == 0 ? t.xs : t.h[l];
    const int ldi = l == 0 ? a.Dp : a.dims[l] + 1;
    dense_fwd(in, ldi, a.dims[l], t.W[l], t.ldw[l], a.b[l], a.dims[l + 1], t.h[l + 1],
              a.dims[l + 1] + 1, lane);
    wave_sync();
  }
}

// Last layer on lanes 0..15 (one row each): logits, then either the label (argmax, first on a
// tie) or the cross-entropy from the logits and d loss / d logit = softmax - onehot.
__device__ __forceinline__ void last_layer(const PgdArgs& a, const PgdTile& t, int lane,
                                           bool predict) {
  const int L = a.n_layers;
  const int K = a.dims[L - 1], no = a.dims[L];
  if (lane < PGD_ROWS) {
    const float* hr = t.h[L - 1] + lane * (K + 1);
    const float* W = t.W[L - 1];
    const int ldw = t.ldw[L - 1];
    float z[PGD_MAX_OUT];
    float mx = -__builtin_inff();
    int am = 0;
#pragma unroll
    for (int c = 0; c < PGD_MAX_OUT; ++c) {
      z[c] = 0.f;
      if (c < no) {
        float s = 0.f;
        for (int k = 0; k < K; ++k) s = fmaf(hr[k], W[k * ldw + c], s);
        z[c] = s + a.b[L - 1][c];
        if (z[c] > mx) {
          mx = z[c];
          am = c;
        }
      }
    }
    if (predict) {
      t.ys[lane] = am;
    } else {
      const int y = t.ys[lane];
      float e[PGD_MAX_OUT];
      float S = 0.f, zy = 0.f;
#pragma unroll
      for (int c = 0; c < PGD_MAX_OUT; ++c) {
        e[c] = 0.f;
        if (c < no) {
          e[c] = expf(z[c] - mx);
          S = S + e[c];
          if (c == y) zy = z[c];
        }
      }
      t.lossc[lane] = -((zy - mx) - logf(S));
#pragma unroll
      for (int c = 0; c < PGD_MAX_OUT; ++c)
        if (c < no) t.dl[lane * PGD_MAX_OUT + c] = e[c] / S - (c == y ? 1.f : 0.f);
    }
  }
  wave_sync();
}

// Backward: t.dl -> t.gs (d CE / d scaled x).
__device__ __forceinline__ void mlp_backward(const PgdArgs& a, const PgdTile& t, int lane) {
  const int L = a.n_layers;
  const int ka = lane >> 4, il = lane & 15;
  const int hm1 = pgd_hmax(a) + 1;
  {  // last layer: dz[row][k] = sum_c dl[row][c] W[k][c], masked by h[L-1] > 0
    const int K = a.dims[L - 1], no = a.dims[L];
    const float* W = t.W[L - 1];
    const int ldw = t.ldw[L - 1];
    for (int k = ka; k < K; k += 4) {
      float s = 0.f;
      for (int c = 0; c < no; ++c) s = fmaf(t.dl[il * PGD_MAX_OUT + c], W[k * ldw + c], s);
      t.dz[0][il * hm1 + k] = t.h[L - 1][il * (K + 1) + k] > 0.f ? s : 0.f;
    }
    wave_sync();
  }
  int cur = 0;
  for (int l = L - 2; l >= 0; --l) {
    if (l > 0) {
      dense_bwd(t.dz[cur], hm1, a.dims[l + 1], t.W[l], t.ldw[l], a.dims[l], t.h[l],
                a.dims[l] + 1, t.dz[cur ^ 1], hm1, lane);
      cur ^= 1;
    } else {
      dense_bwd(t.dz[cur], hm1, a.dims[1], t.W[0], t.ldw[0], a.D, nullptr, 0, t.gs, a.Dp, lane);
    }
    wave_sync();
  }
}

// TF floormod(f, 100): the result has the divisor's sign.
__device__ __forceinline__ float floormod100(float f) {
  float r = fmodf(f, 100.f);
  if (r != 0.f && r < 0.f) r = r + 100.f;
  return r;
}
__device__ __forceinline__ float month_of(float f) {
  return floorf(f / 100.f) * 12.f + floormod100(f);
}

// The installment formula x0 r q / (q - 1), q = (1 + r)^t, r = x2 / 1200, in the reference's
// order (lcld_constraints.py:87-97); dx0 / dr receive its partial derivatives.
__device__ __forceinline__ float installment(float x0, float r, float t, float* dx0, float* dr) {
  const float q = powf(1.f + r, t);
  const float qm = q - 1.f;
  const float inst = x0 * r * q / qm;
  if (dx0) {
    const float dq = t * q / (1.f + r);
    *dx0 = r * q / qm;
    *dr = x0 * (q / qm - r * dq / (qm * qm));
  }
  return inst;
}

// Tensor-path constraint columns of one row (lanes 0..15, lane = row) and the reverse sweep:
// v_j = max(c_j - tol, 0); with `back`, gs[row][f] += -(d v_j / d xf_f) / scale_f for every
// active column (c_j - tol > 0).  Kinks follow TF: abs'(0) = 0, relu'(0) = 0, floor' = 0,
// floormod' = 1, minimum gives the gradient to the smaller argument (the first on a tie).
// cols (or nullptr): global row of 2 + C losses, columns written at cols[2 + j].
// EXPR: the program may hold MV_OP_EXPR columns; tp is the lane's tape column.
template <bool EXPR>
__device__ __forceinline__ float constraint_sweep(const PgdArgs& a, const float* xr, float* gr,
                                                  bool back, float* cols, float* tp) {
  const float* __restrict__ sc = a.scale;
  const float* __restrict__ mn = a.minv;
#define XF(f) ((xr[(f)] - mn[(f)]) / sc[(f)])
#define ADDG(f, coef) gr[(f)] = gr[(f)] + (coef) / sc[(f)]
  float sum = 0.f;
  for (int j = 0; j < a.C; ++j) {
    const int code = a.op_code[j];
    const int a0 = a.op_arg[4 * j], a1 = a.op_arg[4 * j + 1], a2 = a.op_arg[4 * j + 2],
              a3 = a.op_arg[4 * j + 3];
    const float k0 = a.op_k[2 * j];
    if (EXPR && code == MV_OP_EXPR) {  // a0: first instruction, a1: instruction count
      const int4* ins = a.xins + a0;
      const float ct = expr_forward(a, ins, a1, xr, tp) - a.tol;
      const bool active = ct > 0.f;
      const float v = active ? ct : (ct != ct ? ct : 0.f);
      if (cols) cols[2 + j] = v;
      sum = sum + v;
      if (back && active) expr_reverse(a, ins, a1, gr, tp);
      continue;
    }
    float c = 0.f;
    // up to 4 (feature, d c / d xf) pairs; pooled ops sweep their pool instead
    int gf[4] = {0, 0, 0, 0};
    float gv[4] = {0.f, 0.f, 0.f, 0.f};
    int ng = 0;
    float pool_s = 0.f;
    switch (code) {
      case MV_OP_DIFF: {
        c = XF(a0) - XF(a1);
        gf[0] = a0; gv[0] = 1.f; gf[1] = a1; gv[1] = -1.f; ng = 2;
      } break;
      case MV_OP_ABS_SUMDIFF:
      case MV_OP_TF_ABS_SUMDIFF_OFF: {
        float s1 = 0.f, s2 = 0.f;
        for (int i = a0; i < a1; ++i) s1 = s1 + XF(a.pool[i]);
        for (int i = a1; i < a2; ++i) s2 = s2 + XF(a.pool[i]);
        const float d = s1 - s2;
        c = fabsf(d) - k0;
        pool_s = sgn(d);
      } break;
      case MV_OP_TF_INSTALL_MIN: {
        const float x0 = XF(a0), r = XF(a2) / 1200.f, x3 = XF(a3);
        float d0a, dra, d0b, drb;
        const float ia = installment(x0, r, 36.f, &d0a, &dra);
        const float ib = installment(x0, r, 60.f, &d0b, &drb);
        const float da = fabsf(x3 - ia), db = fabsf(x3 - ib);
        const bool first = !(db < da);
        c = (first ? da : db) - k0;
        const float s = sgn(first ? x3 - ia : x3 - ib);
        gf[0] = a3; gv[0] = s;
        gf[1] = a0; gv[1] = -s * (first ? d0a : d0b);
        gf[2] = a2; gv[2] = -s * (first ? dra : drb) / 1200.f;
        ng = 3;
        (void)a1;
      } break;
      case MV_OP_TF_HINGE_DIFF: {
        const float p = k0 + XF(a0) - XF(a1);
        c = p > 0.f ? p : (p != p ? p : 0.f);
        if (p > 0.f) {
          gf[0] = a0; gv[0] = 1.f; gf[1] = a1; gv[1] = -1.f; ng = 2;
        }
      } break;
      case MV_OP_TF_TERM_MIN: {
        const float x = XF(a0);
        const float da = fabsf(36.f - x), db = fabsf(60.f - x);
        const bool first = !(db < da);
        c = first ? da : db;
        gf[0] = a0; gv[0] = -sgn(first ? 36.f - x : 60.f - x); ng = 1;
      } break;
      case MV_OP_ABS_RATIO: {
        const float xa = XF(a0), xb = XF(a1), xc = XF(a2);
        const float d = xa - xb / xc;
        c = fabsf(d);
        const float s = sgn(d);
        gf[0] = a0; gv[0] = s;
        gf[1] = a1; gv[1] = -s / xc;
        gf[2] = a2; gv[2] = s * xb / (xc * xc);
        ng = 3;
      } break;
      case MV_OP_MONTHDIFF: {
        const float d = XF(a0) - (month_of(XF(a1)) - month_of(XF(a2)));
        c = fabsf(d);
        const float s = sgn(d);
        gf[0] = a0; gv[0] = s; gf[1] = a1; gv[1] = -s; gf[2] = a2; gv[2] = s; ng = 3;
      } break;
      case MV_OP_TF_RATIO_ALPHA_NEG: {
        const float xa = XF(a0), xb = XF(a1), xc = XF(a2);
        const float broken = xb / xc;
        const float den = xc + k0;
        const bool bad = broken != broken;
        const float d = xa - (bad ? -1.f : xb / den);
        c = fabsf(d);
        const float s = sgn(d);
        gf[0] = a0; gv[0] = s; ng = 1;
        if (!bad) {
          gf[1] = a1; gv[1] = -s / den;
          gf[2] = a2; gv[2] = s * xb / (den * den);
          ng = 3;
        }
      } break;
      case MV_OP_TF_RATIO_ALPHA_ZERO: {
        const float xa = XF(a0), xb = XF(a1);
        const float broken = xa - xb;
        const float den = xb + k0;
        const bool bad = broken != broken;
        c = bad ? 0.f : xa / den;
        if (!bad) {
          gf[0] = a0; gv[0] = 1.f / den;
          gf[1] = a1; gv[1] = -xa / (den * den);
          ng = 2;
        }
      } break;
      default:
        break;
    }
    const float ct = c - a.tol;
    const bool active = ct > 0.f;
    const float v = active ? ct : (ct != ct ? ct : 0.f);
    if (cols) cols[2 + j] = v;
    sum = sum + v;
    if (back && active) {
      if (code == MV_OP_ABS_SUMDIFF || code == MV_OP_TF_ABS_SUMDIFF_OFF) {
        for (int i = a0; i < a1; ++i) ADDG(a.pool[i], -pool_s);
        for (int i = a1; i < a2; ++i) ADDG(a.pool[i], pool_s);
      } else {
#pragma unroll
        for (int g = 0; g < 4; ++g)
          if (g < ng) ADDG(gf[g], -gv[g]);
      }
    }
  }
#undef XF
#undef ADDG
  return sum;
}

// fix_features_types on one feature-space row (lcld_constraints.py:40-66): term snapped to
// {36, 60}, installment recomputed, every one-hot group set to one-hot at its argmax (first
// maximum, numpy argmax).  stride: distance between a row's features.
__device__ __forceinline__ void repair_row(const PgdArgs& a, float* xr) {
  if (a.inst[0] >= 0) {
    const float x1 = xr[a.inst[1]] < 48.f ? 36.f : 60.f;
    xr[a.inst[1]] = x1;
    const float r = xr[a.inst[2]] / 1200.f;
    xr[a.inst[3]] = installment(xr[a.inst[0]], r, x1, nullptr, nullptr);
  }
  for (int g = 0; g < a.n_ohe; ++g) {
    const int o0 = a.ohe_off[g], o1 = a.ohe_off[g + 1];
    int best = o0;
    float bv = xr[a.ohe_feat[o0]];
    bool nan = bv != bv;
    for (int i = o0 + 1; i < o1 && !nan; ++i) {
      const float v = xr[a.ohe_feat[i]];
      if (v != v) {  // numpy argmax returns the first NaN
        best = i;
        nan = true;
      } else if (v > bv) {
        bv = v;
        best = i;
      }
    }
    for (int i = o0; i < o1; ++i) xr[a.ohe_feat[i]] = i == best ? 1.f : 0.f;
  }
}

__device__ __forceinline__ float row_sum4(float v) {
  v = v + __shfl_xor(v, 16);
  v = v + __shfl_xor(v, 32);
  return v;
}

// One PGD iteration's update on the tile (atk.py:74-163): lane (row = lane & 15, part = lane
// >> 4) walks features part, part + 4, ...
__device__ __forceinline__ void pgd_step(const PgdArgs& a, const PgdTile& t, int lane, int row0,
                                         float eta) {
  const int row = lane & 15, part = lane >> 4;
  const int grow = row0 + row;
  const bool live = grow < a.n;
  float* xr = t.xs + row * a.Dp;
  float* gr = t.gs + row * a.Dp;
  const float* x0 = a.x_in + (size_t)(live ? grow : 0) * a.D;
  const bool l2 = a.norm == 2;
  float ss = 0.f;
  for (int f = part; f < a.D; f += 4) {
    float g = gr[f];
    if (g != g) g = 0.f;
    if (a.mask[f] == 0.f) g = 0.f;
    gr[f] = g;
    ss = ss + g * g;
  }
  const float nrm = sqrtf(row_sum4(ss)) + 1e-7f;
  float dd = 0.f;
  for (int f = part; f < a.D; f += 4) {
    float g = gr[f];
    g = l2 ? g / nrm : sgn(g);
    float x = xr[f] + eta * g;
    x = x < 0.f ? 0.f : (x > 1.f ? 1.f : x);
    const float d = x - (live ? x0[f] : 0.f);
    gr[f] = d;
    dd = dd + d * d;
  }
  const float dn = sqrtf(row_sum4(dd)) + 1e-7f;
  const float q = a.eps / dn;
  const float fac = q < 1.f ? q : 1.f;
  for (int f = part; f < a.D; f += 4) {
    float d = gr[f];
    if (l2) {
      d = d * fac;
    } else {
      const float ad = fabsf(d);
      d = sgn(d) * (ad < a.eps ? ad : a.eps);
    }
    xr[f] = (live ? x0[f] : 0.f) + d;
  }
  wave_sync();
  if (a.repair) {  // x = scale(fix_features_types(unscale(x)))
    for (int f = part; f < a.D; f += 4) xr[f] = (xr[f] - a.minv[f]) / a.scale[f];
    wave_sync();
    if (lane < PGD_ROWS) repair_row(a, t.xs + lane * a.Dp);
    wave_sync();
    for (int f = part; f < a.D; f += 4) xr[f] = xr[f] * a.scale[f] + a.minv[f];
    wave_sync();
  }
}

// The wave's EXPR value tape: the last part of its LDS slice (no PgdTile member, so the
// instances without EXPR columns keep their frame).
__device__ __forceinline__ float* pgd_tape(const PgdTile& t) { return (float*)t.ys + PGD_ROWS; }

// Gradient of the selected loss wrt the scaled rows into t.gs; returns (lanes 0..15) the
// constraint sum.  cols: this lane's global losses row or nullptr.
template <bool EXPR>
__device__ __forceinline__ float pgd_gradient(const PgdArgs& a, const PgdTile& t, int lane,
                                              bool want_class, float* cols) {
  const bool flip = (a.loss_flags & PGD_LOSS_FLIP) != 0;
  const bool cons = (a.loss_flags & PGD_LOSS_CONSTRAINTS) != 0;
  if (flip || want_class) {
    mlp_forward(a, t, lane);
    last_layer(a, t, lane, false);
  }
  if (flip) {
    mlp_backward(a, t, lane);
  } else {
    const int row = lane & 15, part = lane >> 4;
    for (int f = part; f < a.D; f += 4) t.gs[row * a.Dp + f] = 0.f;
    wave_sync();
  }
  float sum = 0.f;
  if (cons || cols) {
    if (lane < PGD_ROWS)
      sum = constraint_sweep<EXPR>(a, t.xs + lane * a.Dp, t.gs + lane * a.Dp, cons, cols,
                                   EXPR ? pgd_tape(t) + lane : nullptr);
    wave_sync();
  }
  return sum;
}

// Carve the dynamic LDS block: weights first (shared by the workgroup), then the waves' tiles.
template <bool EXPR>
__device__ __forceinline__ void pgd_setup(const PgdArgs& a, float* smem, PgdTile& t) {
  float* p = smem;
  for (int l = 0; l < a.n_layers; ++l) {
    const int K = a.dims[l], N = a.dims[l + 1];
    if (l == 0 && !a.stage_w0) {
      t.W[l] = a.W[l];
      t.ldw[l] = N;
      continue;
    }
    const int ld = N + 1;
    for (int i = threadIdx.x; i < K * N; i += blockDim.x) p[(i / N) * ld + i % N] = a.W[l][i];
    t.W[l] = p;
    t.ldw[l] = ld;
    p += K * ld;
  }
  __syncthreads();
  const int hm1 = pgd_hmax(a) + 1;
  size_t per = (size_t)2 * PGD_ROWS * a.Dp + 2 * PGD_ROWS * hm1 + PGD_ROWS * PGD_MAX_OUT + 2 * PGD_ROWS;
  for (int l = 1; l < a.n_layers; ++l) per += (size_t)PGD_ROWS * (a.dims[l] + 1);
  if (EXPR) per += (size_t)PGD_ROWS * a.tape;
  p += per * (threadIdx.x >> 6);
  t.xs = p; p += PGD_ROWS * a.Dp;
  t.gs = p; p += PGD_ROWS * a.Dp;
  for (int l = 1; l < a.n_layers; ++l) {
    t.h[l] = p;
    p += PGD_ROWS * (a.dims[l] + 1);
  }
  t.dz[0] = p; p += PGD_ROWS * hm1;
  t.dz[1] = p; p += PGD_ROWS * hm1;
  t.dl = p; p += PGD_ROWS * PGD_MAX_OUT;
  t.lossc = p; p += PGD_ROWS;
  t.ys = (int*)p;
}


// rows row0 .. row0 + 15 of x_in into t.xs (rows past n: zeros), labels into t.ys
__device__ __forceinline__ void pgd_load(const PgdArgs& a, const PgdTile& t, int lane, int row0) {
  for (int r = 0; r < PGD_ROWS; ++r) {
    const bool live = row0 + r < a.n;
    for (int f = lane; f < a.D; f += 64)
      t.xs[r * a.Dp + f] = live ? a.x_in[(size_t)(row0 + r) * a.D + f] : 0.f;
  }
  if (lane < PGD_ROWS) {
    int y = 0;
    if (a.y && row0 + lane < a.n) {
      y = a.y[row0 + lane];
      y = y < 0 ? 0 : (y >= a.dims[a.n_layers] ? a.dims[a.n_layers] - 1 : y);
    }
    t.ys[lane] = y;
  }
  wave_sync();
}

}  // namespace

template <bool EXPR>
__global__ __launch_bounds__(64 * PGD_MAX_WAVES) void k_pgd(const PgdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float pgd_smem[];
  PgdTile t;
  pgd_setup<EXPR>(a, pgd_smem, t);
  const int lane = threadIdx.x & 63;
  const int row0 = (blockIdx.x * a.wpb + (threadIdx.x >> 6)) * PGD_ROWS;
  if (row0 >= a.n) return;
  pgd_load(a, t, lane, row0);
  if (!a.y) {  // labels: the model's own prediction on the clean rows
    mlp_forward(a, t, lane);
    last_layer(a, t, lane, true);
  }
  for (int it = 0; it < a.max_iter; ++it) {
    pgd_gradient<EXPR>(a, t, lane, false, nullptr);
    float eta = a.eps_step;
    if (a.adaptive) {
      int p = it / a.iter_per_step;
      p = p < PGD_ETA_TAB ? p : PGD_ETA_TAB - 1;
      eta = a.eta_tab[p];
    }
    pgd_step(a, t, lane, row0, eta);
  }
  for (int r = 0; r < PGD_ROWS; ++r) {
    if (row0 + r < a.n)
      for (int f = lane; f < a.D; f += 64)
        a.x_out[(size_t)(row0 + r) * a.D + f] = t.xs[r * a.Dp + f];
  }
}

// One gradient evaluation: grad [n][D] (raw: before mask and normalisation), losses
// [n][2 + C] = (loss_class, constraint sum, the C columns).
template <bool EXPR>
__global__ __launch_bounds__(64 * PGD_MAX_WAVES) void k_pgd_grad(const PgdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float pgd_smem[];
  PgdTile t;
  pgd_setup<EXPR>(a, pgd_smem, t);
  const int lane = threadIdx.x & 63;
  const int row0 = (blockIdx.x * a.wpb + (threadIdx.x >> 6)) * PGD_ROWS;
  if (row0 >= a.n) return;
  pgd_load(a, t, lane, row0);
  float* cols = nullptr;
  if (lane < PGD_ROWS && row0 + lane < a.n && a.losses)
    cols = a.losses + (size_t)(row0 + lane) * (2 + a.C);
  const float sum = pgd_gradient<EXPR>(a, t, lane, true, cols);
  if (cols) {
    cols[0] = t.lossc[lane];
    cols[1] = sum;
  }
  if (a.grad) {
    for (int r = 0; r < PGD_ROWS; ++r) {
      if (row0 + r < a.n)
        for (int f = lane; f < a.D; f += 64)
          a.grad[(size_t)(row0 + r) * a.D + f] = t.gs[r * a.Dp + f];
    }
  }
}

__global__ void k_pgd_repair(const PgdArgs a, float* x) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < a.n) repair_row(a, x + (size_t)r * a.D);
}

static size_t pgd_wave_floats(const PgdArgs& a) {
  int hm = 16;
  for (int l = 1; l < a.n_layers; ++l) hm = a.dims[l] > hm ? a.dims[l] : hm;
  size_t per = (size_t)2 * PGD_ROWS * a.Dp + 2 * PGD_ROWS * (hm + 1) + PGD_ROWS * PGD_MAX_OUT +
               2 * PGD_ROWS;
  for (int l = 1; l < a.n_layers; ++l) per += (size_t)PGD_ROWS * (a.dims[l] + 1);
  per += (size_t)PGD_ROWS * a.tape;  // the EXPR value tape (0 without an EXPR column)
  return per;
}

static size_t pgd_weight_floats(const PgdArgs& a) {
  size_t w = 0;
  for (int l = 0; l < a.n_layers; ++l)
    if (l > 0 || a.stage_w0) w += (size_t)a.dims[l] * (a.dims[l + 1] + 1);
  return w;
}

size_t pgd_lds_bytes(const PgdArgs& a) {
  return (pgd_weight_floats(a) + pgd_wave_floats(a) * (size_t)a.wpb) * sizeof(float);
}

// Tiles per workgroup: as many as fill the device once (256 CUs) and fit in LDS.
static hipError_t pgd_plan(PgdArgs& a) {
  const int tiles = (a.n + PGD_ROWS - 1) / PGD_ROWS;
  int wpb = tiles / 256;
  wpb = wpb < 1 ? 1 : (wpb > PGD_MAX_WAVES ? PGD_MAX_WAVES : wpb);
  a.wpb = wpb;
  while (a.wpb > 1 && pgd_lds_bytes(a) > (size_t)PGD_LDS_BYTES) --a.wpb;
  if (pgd_lds_bytes(a) > (size_t)PGD_LDS_BYTES) return hipErrorInvalidValue;
  return hipSuccess;
}

template <class Kern>
static hipError_t pgd_launch(Kern kern, PgdArgs a, hipStream_t stream) {
  if (a.n <= 0) return hipSuccess;
  hipError_t e = pgd_plan(a);
  if (e != hipSuccess) return e;
  const size_t lds = pgd_lds_bytes(a);
  if (lds > 64 * 1024) {  // per device: set on every large launch (a host-side table write)
    e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                            PGD_LDS_BYTES);
    if (e != hipSuccess) return e;
  }
  const int tiles = (a.n + PGD_ROWS - 1) / PGD_ROWS;
  const int blocks = (tiles + a.wpb - 1) / a.wpb;
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(64 * a.wpb), lds, stream, a);
  return hipGetLastError();
}

// a.tape > 0: the program has an EXPR column (mv_pgd_create) and runs the <true> instances
hipError_t launch_pgd(const PgdArgs& a, hipStream_t stream) {
  return a.tape > 0 ? pgd_launch(k_pgd<true>, a, stream) : pgd_launch(k_pgd<false>, a, stream);
}

hipError_t launch_pgd_grad(const PgdArgs& a, hipStream_t stream) {
  return a.tape > 0 ? pgd_launch(k_pgd_grad<true>, a, stream)
                    : pgd_launch(k_pgd_grad<false>, a, stream);
}

hipError_t launch_pgd_repair(const PgdArgs& a, float* x, hipStream_t stream) {
  if (a.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_pgd_repair, dim3((a.n + 127) / 128), dim3(128), 0, stream, a, x);
  return hipGetLastError();
}

MV_DEFINE_TAKE_CHECKS(take_checks_pgd)

}  // namespace mv
