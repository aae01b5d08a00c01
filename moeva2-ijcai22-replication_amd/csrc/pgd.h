// C-PGD (constrained projected gradient descent) on device: launch interface of pgd.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace mv {

constexpr int PGD_MAX_LAYERS = 6;
constexpr int PGD_ROWS = 16;       // rows per tile: one wave owns one tile
constexpr int PGD_MAX_WAVES = 4;   // tiles per workgroup
constexpr int PGD_MAX_OUT = 8;     // classes
constexpr int PGD_ETA_TAB = 16;    // adaptive step table (iter / (max_iter / 7) < 14)
constexpr int PGD_LDS_BYTES = 160 * 1024;

// loss_flags
constexpr int PGD_LOSS_FLIP = 1;         // + cross-entropy of the logits
constexpr int PGD_LOSS_CONSTRAINTS = 2;  // - sum of the tensor-path constraint columns

struct PgdArgs {
  // problem (device tables, fp32)
  int D, C, n_layers;
  int dims[PGD_MAX_LAYERS + 1];
  const float* W[PGD_MAX_LAYERS];  // [dims[l]][dims[l+1]] row-major
  const float* b[PGD_MAX_LAYERS];
  const float* scale;              // [D] ML MinMaxScaler scale_
  const float* minv;               // [D] min_
  const float* mask;               // [D] 1 = mutable
  const int* op_code;              // [C]
  const int* op_arg;               // [C][4]
  const float* op_k;               // [C][2]
  const int* pool;
  int n_ohe;
  const int* ohe_off;              // [n_ohe+1]
  const int* ohe_feat;
  int inst[4];                     // repair: amount, term, rate, installment features (inst[0] < 0: none)
  float tol;
  // LDS plan
  int Dp;                          // row stride of the x / gradient tiles (odd)
  int stage_w0;                    // first layer staged in LDS (else streamed from L2)
  int wpb;                         // waves (tiles) per workgroup
  // call
  int n;
  const float* x_in;               // [n][D] scaled rows
  const int* y;                    // [n] labels or nullptr (model's own prediction)
  float* x_out;                    // [n][D]
  int max_iter, norm, loss_flags, adaptive, repair, iter_per_step;
  float eps, eps_step;
  float eta_tab[PGD_ETA_TAB];
  float* grad;                     // k_pgd_grad: [n][D] raw gradient
  float* losses;                   // k_pgd_grad: [n][2 + C]
  // MV_OP_EXPR columns (pgd_expr.h); a program without one leaves these zero and runs the
  // kernels without the interpreter
  const int4* xins;                // decoded instructions of all EXPR columns; an EXPR column's
                                   // op_arg = (first instruction, instruction count, 0, 0)
  const float* xk;                 // their constants, rounded to fp32 once on the host
  int tape;                        // largest column's instruction count (0: no EXPR column):
                                   // the per-wave tape is [tape][PGD_ROWS] floats of LDS
};

size_t pgd_lds_bytes(const PgdArgs& a);
hipError_t launch_pgd(const PgdArgs& a, hipStream_t stream);
hipError_t launch_pgd_grad(const PgdArgs& a, hipStream_t stream);
// fix_features_types on feature-space rows x [n][D], in place
hipError_t launch_pgd_repair(const PgdArgs& a, float* x, hipStream_t stream);

}  // namespace mv
