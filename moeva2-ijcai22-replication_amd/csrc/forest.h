// Tree-ensemble classifiers on the device (forest.hip k_forest): scikit-learn's predict_proba
// for RandomForestClassifier / ExtraTreesClassifier / DecisionTreeClassifier, restated in
// moeva2_amd/models/forest.py (predict_proba_numpy, the specification).
//
// The host checks a forest's tables (api.cpp forest_check: 2..8 classes, features in [0, D),
// every child inside its own tree and after its parent, so a walk cannot cycle) and packs
// them (forest_pack) before anything is uploaded: the device only walks checked tables.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mv {

constexpr int FOREST_MAX_CLASSES = 8;
constexpr int FOREST_T = 64;  // threads per k_forest workgroup: one wave, one row per lane

// One node, 16 bytes (one dwordx4 load).  The nodes of a tree are renumbered breadth first
// so that siblings are neighbours: right child = left + 1.
//   slot >= 0: an inner node; the tested value lives at `slot` (below); go to `left` when
//              (double)value <= threshold, else to left + 1
//   slot <  0: a leaf; its row is leaf_value[~slot]
// Engine rows (k_forest<true>): slot < Dm4 is an index into the row's fp32 ML row (xml, the
// mutable features the row kernels write), slot >= Dm4 is feature slot - Dm4 of the state's
// fp32 vector xfix (the features the attack does not move).  mv_forest_predict
// (k_forest<false>): slot is the feature itself.
struct ForestNode {
  double threshold;
  int slot;
  int left;
};
static_assert(sizeof(ForestNode) == 16, "a node is one 16-byte load");

struct DForest {
  const ForestNode* nodes;   // [n_nodes]
  const int* tree_root;      // [n_trees]
  const double* leaf_value;  // [n_leaves][n_classes]: value / normalizer, from the host
  int n_nodes, n_trees, n_leaves, n_classes;  // n_trees == 0: no forest
};

struct ForestArgs {
  DForest f;
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

hipError_t launch_forest_rows(const ForestArgs& a, hipStream_t stream);
hipError_t launch_forest_predict(const ForestArgs& a, hipStream_t stream);

}  // namespace mv
