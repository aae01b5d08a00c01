// k_forest: a tree ensemble's predict_proba, one lane per row (gfx950).
//
// Each lane walks every tree in order and keeps the class sums in registers: fp64 sums of the
// trees' leaf rows in tree order starting from 0.0, divided by the number of trees -- the
// operations of predict_proba_numpy (moeva2_amd/models/forest.py), so the result has its bits.
// A node is one 16-byte load (forest.h ForestNode); the nodes stay in global memory (a
// 100-tree forest of 1,000-node trees is 1.6 MB: L2).  Lanes diverge per tree.
//
// ROWS: the engine's fitness path (launch_mlp's FOREST_ROWS route) -- the tested value comes
// from the row's fp32 ML row or, for a feature the attack does not move, from the state's
// xfix; writes f1 = proba[min_class] into F[..][0] and the history.  Otherwise
// mv_forest_predict: fp64 ML-scaled rows, cast to fp32 as sklearn casts X; writes proba.
#include "check.h"
#include "forest.h"
#include "kernels.h"

namespace mv {

template <bool ROWS>
__global__ __launch_bounds__(FOREST_T) void k_forest(const ForestArgs a) {
  const int r = blockIdx.x * FOREST_T + threadIdx.x;
  if (r >= a.total) return;
  const DForest& f = a.f;
  const int st = ROWS ? r / a.n : 0;
  const float* xr = a.xml + (ROWS ? (size_t)r * a.Dm4 : 0);
  const float* xf = a.xfix + (ROWS ? (size_t)st * a.D : 0);
  const double* xp = a.x + (ROWS ? 0 : (size_t)r * a.D);
  const int4* nodes = (const int4*)f.nodes;
  const int nc = f.n_classes;
  double s[FOREST_MAX_CLASSES];
#pragma unroll
  for (int c = 0; c < FOREST_MAX_CLASSES; ++c) s[c] = 0.0;
  for (int t = 0; t < f.n_trees; ++t) {
    int node = f.tree_root[t];
    int slot;
    for (;;) {  // ends at a leaf: every child index is greater than its parent's (host check)
      const int4 w = nodes[MV_IDX(node, f.n_nodes, CK_FOREST_NODE)];
      slot = w.z;
      if (slot < 0) break;
      float v;
      if (ROWS)
        v = slot < a.Dm4 ? xr[slot] : xf[MV_IDX(slot - a.Dm4, a.D, CK_FOREST_SLOT)];
      else
        v = (float)xp[MV_IDX(slot, a.D, CK_FOREST_SLOT)];
      const double thr = __hiloint2double(w.y, w.x);
      node = w.w + ((double)v <= thr ? 0 : 1);  // a NaN goes right
    }
    const double* lv = f.leaf_value + (size_t)MV_IDX(~slot, f.n_leaves, CK_FOREST_LEAF) * nc;
#pragma unroll
    for (int c = 0; c < FOREST_MAX_CLASSES; ++c)
      if (c < nc) s[c] = s[c] + lv[c];
  }
  const double nt = (double)f.n_trees;
  if (ROWS) {
    const int mc = a.min_class[st];
    double v = s[0];
#pragma unroll
    for (int c = 1; c < FOREST_MAX_CLASSES; ++c) v = mc == c ? s[c] : v;
    const double f1 = v / nt;
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
    for (int c = 0; c < FOREST_MAX_CLASSES; ++c)
      if (c < nc) out[c] = s[c] / nt;
  }
}

template <bool ROWS>
static hipError_t launch_forest(const ForestArgs& a, hipStream_t stream) {
  if (a.total <= 0) return hipSuccess;
  if (a.f.n_trees <= 0 || a.f.n_classes < 2 || a.f.n_classes > FOREST_MAX_CLASSES)
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)((a.total + FOREST_T - 1) / FOREST_T));
  MV_LAUNCH(k_forest<ROWS>, grid, dim3(FOREST_T), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_forest_rows(const ForestArgs& a, hipStream_t stream) {
  if (!a.xml || !a.xfix || !a.min_class || a.n <= 0) return hipErrorInvalidValue;
  return launch_forest<true>(a, stream);
}

hipError_t launch_forest_predict(const ForestArgs& a, hipStream_t stream) {
  return launch_forest<false>(a, stream);
}

MV_DEFINE_TAKE_CHECKS(take_checks_forest)

}  // namespace mv
