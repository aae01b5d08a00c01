// k_svm: a kernel machine's or a logistic regression's predict_proba, one lane per row (gfx950).
//
// The work is rows x vectors x features of fp64 fma.  A lane keeps SVM_FC features of its row
// and SVM_VB vectors' partial sums in registers; the vectors are packed so that the SVM_VB
// entries of one feature are 128 contiguous bytes at a wave-uniform address, which the
// compiler fetches with scalar loads and feeds to v_fma_f64 as SGPR operands: one fetch per
// SVM_VB fma, no LDS, no cross-lane traffic.  For each block of vectors the feature loop runs
// in chunks of SVM_FC with the partial sums carried, so every sum is the chain of svm.h
// whatever D is (756 for botnet) and whatever the launch geometry.  Padding (features past D,
// vectors past n_vec) is zeros on both sides: fma(0, 0, s) = s, and a padded vector's sum is
// never used.
//
// ROWS: the engine's fitness path (launch_mlp's SVM_ROWS route), as k_boost<true>: feature j
// comes from the row's fp32 ML row or the state's xfix by slot[j]; writes f1 = proba[min_class]
// into F[..][0] and the history.  Otherwise mv_forest_predict on an svm handle: fp64 ML-scaled
// rows, cast to fp32; writes proba.
#include "svm.h"

#include "check.h"
#include "kernels.h"

namespace mv {

template <bool RBF>
__device__ __forceinline__ void svm_chunk(const double* __restrict__ vp, const double (&xt)[SVM_FC],
                                          double (&acc)[SVM_VB]) {
#pragma unroll
  for (int jj = 0; jj < SVM_FC; ++jj)
#pragma unroll
    for (int u = 0; u < SVM_VB; ++u) acc[u] = svm_term<RBF>(acc[u], xt[jj], vp[jj * SVM_VB + u]);
}

template <bool ROWS>
__global__ __launch_bounds__(SVM_T) void k_svm(const SvmArgs a) {
  const DSvm& f = a.f;
  const int r = blockIdx.x * SVM_T + threadIdx.x;
  if (r >= a.total) return;  // no barrier follows
  const int st = ROWS ? r / a.n : 0;
  const float* xr = a.xml + (ROWS ? (size_t)r * a.Dm4 : 0);
  const float* xf = a.xfix + (ROWS ? (size_t)st * f.D : 0);
  const double* xp = a.x + (ROWS ? 0 : (size_t)r * f.D);
  const int D = f.D, Dp = f.Dp, nv = f.n_vec, no = f.n_out, nc = f.n_classes;
  const bool rbf = f.kernel == SVM_RBF;

  double xt[SVM_FC];
  // features j0 .. j0 + SVM_FC - 1 of this lane's row as fp64 of their fp32 value; 0 past D
  auto load_tile = [&](int j0) {
#pragma unroll
    for (int jj = 0; jj < SVM_FC; ++jj) {
      const int j = j0 + jj;
      float v;
      if (ROWS) {
        const int s = f.slot[j];  // 0 past D: a valid element, discarded below
        v = s < a.Dm4 ? xr[MV_IDX(s, a.Dm4, CK_SVM_SLOT)] : xf[MV_IDX(s - a.Dm4, D, CK_SVM_SLOT)];
      } else {
        v = (float)xp[j < D ? j : D - 1];
      }
      xt[jj] = j < D ? (double)v : 0.0;
    }
  };
  const bool one_chunk = Dp == SVM_FC;  // the row fits the tile: load it once
  if (one_chunk) load_tile(0);

  double dec[SVM_MAX_CLASSES];
#pragma unroll
  for (int c = 0; c < SVM_MAX_CLASSES; ++c) dec[c] = 0.0;
  for (int v0 = 0; v0 < nv; v0 += SVM_VB) {
    double acc[SVM_VB];
#pragma unroll
    for (int u = 0; u < SVM_VB; ++u) acc[u] = 0.0;
    const double* vb = f.vp + (size_t)(v0 / SVM_VB) * Dp * SVM_VB;
    for (int j0 = 0; j0 < Dp; j0 += SVM_FC) {
      if (!one_chunk) load_tile(j0);
      if (rbf)
        svm_chunk<true>(vb + (size_t)j0 * SVM_VB, xt, acc);
      else
        svm_chunk<false>(vb + (size_t)j0 * SVM_VB, xt, acc);
    }
    // the block's kernel values into the decisions, in vector order
#pragma unroll
    for (int u = 0; u < SVM_VB; ++u) {
      const int v = v0 + u;
      if (v < nv) {  // wave-uniform
        const double k = svm_kernel_value(f.kernel, acc[u], f.gamma, f.coef0, f.degree);
        if (f.coef) {
          for (int o = 0; o < no; ++o) {
            const double t = f.coef[(size_t)o * nv + v] * k;
#pragma unroll
            for (int c = 0; c < SVM_MAX_CLASSES; ++c) dec[c] = c == o ? dec[c] + t : dec[c];
          }
        } else {
#pragma unroll
          for (int c = 0; c < SVM_MAX_CLASSES; ++c) dec[c] = c == v ? k : dec[c];
        }
      }
    }
  }
#pragma unroll
  for (int c = 0; c < SVM_MAX_CLASSES; ++c)
    if (c < no) dec[c] = dec[c] + f.intercept[c];

  double p[SVM_MAX_CLASSES];
#pragma unroll
  for (int c = 0; c < SVM_MAX_CLASSES; ++c) p[c] = 0.0;
  if (f.link == SVM_LINK_PLATT) {
    svm_couple2(svm_platt(dec[0], f.probA, f.probB), p[0], p[1], nullptr);
  } else if (f.link == SVM_LINK_SIGMOID) {
    p[1] = 1.0 / (1.0 + det_exp2(-dec[0], 0.0));
    p[0] = 1.0 - p[1];
  } else {
    double m = dec[0];
#pragma unroll
    for (int c = 1; c < SVM_MAX_CLASSES; ++c)
      if (c < nc) m = dec[c] > m ? dec[c] : m;
    double sum = 0.0;
#pragma unroll
    for (int c = 0; c < SVM_MAX_CLASSES; ++c) {
      p[c] = c < nc ? det_exp2(dec[c] - m, 0.0) : 0.0;
      if (c == 1) sum = p[0] + p[1];  // (e[0] + e[1]) + e[2] + ... in class order
      if (c > 1 && c < nc) sum = sum + p[c];
    }
#pragma unroll
    for (int c = 0; c < SVM_MAX_CLASSES; ++c) p[c] = p[c] / sum;
  }
  if (ROWS) {
    const int mc = a.min_class[st];
    double f1 = p[0];
#pragma unroll
    for (int c = 1; c < SVM_MAX_CLASSES; ++c) f1 = mc == c ? p[c] : f1;
    const int i = r - st * a.n;
    if (a.F) {
      const int orow = MV_IDX(a.out_map ? a.out_map[r] : i, a.out_rows, CK_MLP_OUT);
      a.F[((size_t)st * a.out_rows + orow) * 3] = f1;
    }
    if (a.hist)
      a.hist[((size_t)st * a.hist_rows + MV_IDX(a.hist_row0 + i, a.hist_rows, CK_MLP_OUT)) *
             a.hist_w] = f1;
  } else {
    double* out = a.proba + (size_t)r * nc;
#pragma unroll
    for (int c = 0; c < SVM_MAX_CLASSES; ++c)
      if (c < nc) out[c] = p[c];
  }
}

template <bool ROWS>
static hipError_t launch_svm(const SvmArgs& a, hipStream_t stream) {
  if (a.total <= 0) return hipSuccess;
  const DSvm& f = a.f;
  if (f.n_vec <= 0 || f.D <= 0 || f.Dp < f.D || f.Dp % SVM_FC || f.n_out < 1 ||
      f.n_out > SVM_MAX_CLASSES || f.n_classes < 2 || f.n_classes > SVM_MAX_CLASSES || !f.vp ||
      !f.intercept || (!f.coef && f.n_vec != f.n_out) || (ROWS && !f.slot))
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)((a.total + SVM_T - 1) / SVM_T));
  MV_LAUNCH((k_svm<ROWS>), grid, dim3(SVM_T), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_svm_rows(const SvmArgs& a, hipStream_t stream) {
  if (!a.xml || !a.xfix || !a.min_class || a.n <= 0) return hipErrorInvalidValue;
  return launch_svm<true>(a, stream);
}

hipError_t launch_svm_predict(const SvmArgs& a, hipStream_t stream) {
  if (!a.x || !a.proba) return hipErrorInvalidValue;
  return launch_svm<false>(a, stream);
}

MV_DEFINE_TAKE_CHECKS(take_checks_svm)

}  // namespace mv
