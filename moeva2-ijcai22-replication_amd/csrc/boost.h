// Gradient-boosted tree classifiers on the device (boost.hip k_boost): scikit-learn's
// GradientBoostingClassifier (log-loss) / HistGradientBoostingClassifier predict_proba,
// restated in moeva2_amd/models/boost.py (predict_proba_numpy, the specification).
//
// Tree t adds the scalar of the leaf a row reaches to raw[t % n_outputs], starting from base;
// the raw scores go through a sigmoid (n_outputs == 1: two classes) or a softmax.  The host
// checks the tables with the forest's rules (api.cpp forest_check) plus boost_check's, and
// packs them (forest_pack's order: breadth first, siblings adjacent) before anything is
// uploaded: the device only walks checked tables.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mv {

constexpr int BOOST_MAX_CLASSES = 8;
constexpr int BOOST_T = 64;       // k_boost<.., false>: one wave, one row per lane
constexpr int BOOST_LDS_T = 256;  // k_boost<.., true>: four waves share one copy of the nodes
// The LDS route's budget for the packed nodes.  A CU has 160 KiB; two workgroups of four
// waves per CU (two waves per SIMD: one walks while the other waits on its node) may hold
// 80 KiB each, and 64 KiB is the most a launch takes without asking for a larger limit.
// 4,096 nodes: 100 stages of depth 5, or 270 of depth 3.
constexpr int BOOST_LDS_MAX_BYTES = 64 * 1024;

// One node, 16 bytes (one dwordx4 load); numbering as ForestNode's (right child = left + 1).
//   slot >= 0: an inner node; go to `left` when (double)value_at(slot) <= v, else to left + 1
//              (slot: forest.h ForestNode)
//   slot <  0: a leaf; v is what the tree adds (learning rate included)
struct BoostNode {
  double v;  // threshold, or the leaf's value
  int slot;
  int left;
};
static_assert(sizeof(BoostNode) == 16, "a node is one 16-byte load");

struct DBoost {
  const BoostNode* nodes;  // [n_nodes]
  const int* tree_root;    // [n_trees]
  const double* base;      // [n_outputs]
  int n_nodes, n_trees, n_classes, n_outputs;  // n_trees == 0: no boosted ensemble
};

__host__ __device__ inline bool boost_lds_ok(const DBoost& b) {
  return (long long)b.n_nodes * (long long)sizeof(BoostNode) <= BOOST_LDS_MAX_BYTES;
}

struct BoostArgs {
  DBoost f;
  int total;  // rows
  int D;
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

// lds: the BOOST_ROWS_LDS route (the caller has checked boost_lds_ok)
hipError_t launch_boost_rows(const BoostArgs& a, bool lds, hipStream_t stream);
hipError_t launch_boost_predict(const BoostArgs& a, bool lds, hipStream_t stream);

}  // namespace mv
