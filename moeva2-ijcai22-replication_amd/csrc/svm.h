// Kernel machines and logistic regression on the device (svm.hip k_svm): scikit-learn's
// SVC / NuSVC (probability=True, two classes) and LogisticRegression predict_proba, restated in
// moeva2_amd/models/svm.py (predict_proba_numpy, the specification).
//
// A model is n_vec vectors of D features, a kernel K(x, v) (linear, poly, rbf), a coefficient
// matrix coef[n_out][n_vec] (or none: the decision is K itself, logistic regression) and a link
// from the decisions to probabilities (Platt's sigmoid with libsvm's pairwise coupling, a
// sigmoid, a softmax).  The host checks the tables (api.cpp svm_check) and packs the vectors
// (svm_pack) before anything is uploaded.
//
// The arithmetic is one fixed sequence per row, whatever the launch:
//   s_v     = 0, then over features j ascending: s_v = svm_term(s_v, x_j, v_j)   (one fma each)
//   K_v     = svm_kernel_value(s_v)
//   dec[o]  = 0, then over vectors v ascending: dec[o] = dec[o] + coef[o][v] * K_v (mul, add),
//             then dec[o] = dec[o] + intercept[o]        (no coef: dec[o] = K_o + intercept[o])
//   proba   = the link of dec
// svm_term, svm_kernel_value and the links are __host__ __device__ inline here, and mv_svm_sums
// exports the host build of the feature sums: the specification calls it, as it calls
// mv_det_exp, so host and device run the same IEEE operations.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "detmath.h"

namespace mv {

constexpr int SVM_MAX_CLASSES = 8;
constexpr int SVM_T = 64;   // one wave per workgroup, one row per lane
// The register tile of a lane: SVM_FC features of its row (fp64: 32 VGPRs) against SVM_VB
// vectors' partial sums (32 VGPRs).  One 128-byte scalar fetch (the SVM_VB entries of one
// feature) feeds SVM_VB v_fma_f64; one row load of SVM_FC floats feeds SVM_FC * SVM_VB.
constexpr int SVM_FC = 16;  // features per chunk
constexpr int SVM_VB = 16;  // vectors per block
// n_vec * D (unpadded) the engine accepts: 2^24 entries, 128 MiB of fp64
constexpr long long SVM_MAX_ENTRIES = 1ll << 24;
constexpr int SVM_MAX_DEGREE = 64;

enum SvmKernel : int { SVM_LINEAR = 0, SVM_POLY = 1, SVM_RBF = 2 };
enum SvmLink : int {
  SVM_LINK_PLATT = 0,    // SVC / NuSVC, two classes: Platt's sigmoid, libsvm's coupling
  SVM_LINK_SIGMOID = 1,  // logistic regression, two classes
  SVM_LINK_SOFTMAX = 2,  // logistic regression, 3..8 classes
};

// One feature's term of the sum a kernel needs: x.v (linear, poly) or |x - v|^2 (rbf).
template <bool RBF>
__host__ __device__ inline double svm_term(double acc, double x, double v) {
  if (RBF) {
    const double d = x - v;
    return fma(d, d, acc);
  }
  return fma(x, v, acc);
}

// libsvm's powi: square-and-multiply over the bits of the degree
__host__ __device__ inline double svm_powi(double base, int times) {
  double tmp = base, ret = 1.0;
  for (int t = times; t > 0; t /= 2) {
    if (t % 2 == 1) ret = ret * tmp;
    tmp = tmp * tmp;
  }
  return ret;
}

// K(x, v) from the feature sum s
__host__ __device__ inline double svm_kernel_value(int kernel, double s, double gamma,
                                                   double coef0, int degree) {
  if (kernel == SVM_RBF) return det_exp2(-(gamma * s), 0.0);
  if (kernel == SVM_POLY) return svm_powi(gamma * s + coef0, degree);
  return s;
}

// libsvm's sigmoid_predict on its own decision value (the opposite sign of sklearn's
// decision_function), clipped as svm_predict_probability clips it: max and min as libsvm's
// macros write them, so a NaN becomes 1e-7.
__host__ __device__ inline double svm_platt(double dec, double probA, double probB) {
  const double f = (-dec) * probA + probB;
  double s;
  if (f >= 0) {
    const double e = det_exp2(-f, 0.0);
    s = e / (1.0 + e);
  } else {
    s = 1.0 / (1.0 + det_exp2(f, 0.0));
  }
  const double lo = 1e-7, hi = 1 - 1e-7;
  s = s > lo ? s : lo;
  return s < hi ? s : hi;
}

// libsvm's multiclass_probability for k = 2 from r01 (r10 = 1 - r01): at most 100 iterations,
// eps = 0.005 / 2.  A NaN ends the loop at its first test (no comparison with it is true).
__host__ __device__ inline void svm_couple2(double r01, double& p0, double& p1, int* iters) {
  const double r10 = 1.0 - r01;
  const double q00 = r10 * r10, q01 = -r10 * r01, q11 = r01 * r01, eps = 0.005 / 2;
  p0 = 0.5;
  p1 = 0.5;
  int it = 0;
  for (; it < 100; ++it) {
    double qp0 = q00 * p0 + q01 * p1;
    double qp1 = q01 * p0 + q11 * p1;
    double pqp = p0 * qp0 + p1 * qp1;
    const double e0 = fabs(qp0 - pqp), e1 = fabs(qp1 - pqp);
    double err = 0.0;
    if (e0 > err) err = e0;
    if (e1 > err) err = e1;
    if (err < eps) break;
    {  // t = 0
      const double diff = (-qp0 + pqp) / q00;
      p0 = p0 + diff;
      pqp = (pqp + diff * (diff * q00 + 2 * qp0)) / (1 + diff) / (1 + diff);
      qp0 = (qp0 + diff * q00) / (1 + diff);
      p0 = p0 / (1 + diff);
      qp1 = (qp1 + diff * q01) / (1 + diff);
      p1 = p1 / (1 + diff);
    }
    {  // t = 1
      const double diff = (-qp1 + pqp) / q11;
      p1 = p1 + diff;
      p0 = p0 / (1 + diff);
      p1 = p1 / (1 + diff);
    }
  }
  if (iters) *iters = it;
}

struct DSvm {
  // [n_blocks][Dp][SVM_VB]: entry j of vector SVM_VB * b + u at (b * Dp + j) * SVM_VB + u,
  // zero where j >= D or the vector does not exist (a zero feature adds fma(0, 0, s) = s)
  const double* vp;
  const double* coef;       // [n_out][n_vec], or null: dec[o] = K_o (n_vec == n_out)
  const double* intercept;  // [n_out]
  // engine rows: where feature j of a row lives (forest.h ForestNode's slot), [Dp], 0 past D
  const int* slot;
  int n_vec, n_out, n_classes;  // n_vec == 0: no such model
  int D, Dp;                    // Dp: D rounded up to SVM_FC
  int kernel, degree, link;
  double gamma, coef0, probA, probB;
};

struct SvmArgs {
  DSvm f;
  int total;  // rows
  // engine rows (RowsArgs' fields of the same names)
  int n;
  int Dm4;
  const float* xml;   // [total][Dm4]
  const float* xfix;  // [B][D]
  const int* min_class;
  const int* out_map;
  double* F;
  int out_rows;
  double* hist;
  int hist_rows, hist_w, hist_row0;
  // mv_forest_predict
  const double* x;  // [total][D] ML-scaled rows
  double* proba;    // [total][n_classes]
};

hipError_t launch_svm_rows(const SvmArgs& a, hipStream_t stream);
hipError_t launch_svm_predict(const SvmArgs& a, hipStream_t stream);

}  // namespace mv
