// Training of the Dense MLP on device (adversarial retraining): launch interface of train.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "pgd.h"

namespace mv {

constexpr int TRAIN_MAX_GROUPS = 256;  // workgroups of one batch: rows of the partial scratch

struct TrainArgs {
  // model: dims and the flat parameter vector (per layer W row-major (in, out), then b)
  int D, n_layers;
  int dims[PGD_MAX_LAYERS + 1];
  int off_w[PGD_MAX_LAYERS], off_b[PGD_MAX_LAYERS];
  int n_params;
  const float* params;             // [n_params]
  // LDS plan (train_plan)
  int Dp;                          // row stride of the x tile (odd)
  int stage_w0;                    // first layer staged in LDS (else streamed from L2)
  int wpb;                         // waves per workgroup: tiles worked on at once
  int tpw;                         // tiles per wave: rounds of the workgroup
  int groups;                      // workgroups
  // call: batch row r is row perm[first + r] (perm nullptr: first + r) of x / y
  int n_total;                     // rows of x, y and perm
  int first, n;                    // the batch: n rows from position first
  const float* x;                  // [n_total][D] scaled rows
  const int* y;                    // [n_total] class indices
  const int* perm;                 // [n_total] or nullptr
  float* partial;                  // [groups][n_params] per-workgroup gradient (k_train_grad)
  float* loss_partial;             // [groups][2] per-workgroup (sum of cross-entropy, correct)
};

struct AdamArgs {
  int n_params, groups;
  const float* partial;            // [groups][n_params]
  const float* loss_partial;       // [groups][2]
  float* params;                   // [n_params]; nullptr: no update
  float* m;
  float* v;
  float lr_t, beta1, beta2, epsilon;
  float rows;                      // the batch's row count (loss mean)
  float* grad_out;                 // [n_params] reduced gradient or nullptr
  float* loss_out;                 // [1] mean cross-entropy or nullptr
  float* correct_out;              // [1] argmax-correct rows or nullptr
};

size_t train_lds_bytes(const TrainArgs& a);
// fills stage_w0 (with wpb = tpw = 1): hipErrorInvalidValue when one tile does not fit in LDS
hipError_t train_plan_model(TrainArgs& a);
// forward, backward and the weight gradient of one batch into a.partial / a.loss_partial;
// sets a.wpb, a.tpw, a.groups for a.n rows
hipError_t launch_train_grad(TrainArgs& a, hipStream_t stream);
// forward only: a.loss_partial
hipError_t launch_train_eval(TrainArgs& a, hipStream_t stream);
// fixed-order reduction of the partials, then Adam (params), the gradient (grad_out) or neither
hipError_t launch_train_adam(const AdamArgs& a, hipStream_t stream);

}  // namespace mv
