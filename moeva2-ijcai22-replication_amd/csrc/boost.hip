// k_boost: a gradient-boosted tree ensemble's predict_proba, one lane per row (gfx950).
//
// Each lane keeps the raw scores in registers: raw[k] = base[k], then every tree's leaf value is
// added to raw[t % n_outputs] in tree order in fp64; two classes go through a sigmoid, more
// through a softmax whose exp is detmath.h's det_exp2(x, 0.0) -- the operations of
// predict_proba_numpy (moeva2_amd/models/boost.py, which calls the host build of the same
// function), so the result has its bits.  A node is one 16-byte load (boost.h BoostNode) and a
// leaf carries its value, so a tree of depth d costs d + 1 dependent loads.
//
// LDS: the BOOST_ROWS_LDS route.  Boosted ensembles are many shallow trees (100 stages of
// depth 3 are 1,500 nodes, 24 KB), so a workgroup of four waves copies the packed nodes into
// LDS once, with coalesced 16-byte loads, and walks them there; otherwise the nodes are read
// from global memory (L2).  Lanes diverge per tree on either route.
//
// ROWS: the engine's fitness path (launch_mlp's BOOST_ROWS / BOOST_ROWS_LDS routes), as
// k_forest<true>: the tested value comes from the row's fp32 ML row or the state's xfix; writes
// f1 = proba[min_class] into F[..][0] and the history.  Otherwise mv_forest_predict on a boost
// handle: fp64 ML-scaled rows, cast to fp32; writes proba.
#include "boost.h"
#include "check.h"
#include "detmath.h"
#include "kernels.h"

namespace mv {

template <bool ROWS, bool LDS>
__global__ __launch_bounds__(LDS ? BOOST_LDS_T : BOOST_T) void k_boost(const BoostArgs a) {
  extern __shared__ int4 s_nodes[];
  constexpr int T = LDS ? BOOST_LDS_T : BOOST_T;
  const DBoost& f = a.f;
  const int4* gnodes = (const int4*)f.nodes;
  if (LDS) {  // every lane of the workgroup copies, rows or not; n_nodes fits (launch_boost)
    for (int i = threadIdx.x; i < f.n_nodes; i += T) s_nodes[i] = gnodes[i];
    __syncthreads();
  }
  const int r = blockIdx.x * T + threadIdx.x;
  if (r >= a.total) return;  // no barrier follows
  const int st = ROWS ? r / a.n : 0;
  const float* xr = a.xml + (ROWS ? (size_t)r * a.Dm4 : 0);
  const float* xf = a.xfix + (ROWS ? (size_t)st * a.D : 0);
  const double* xp = a.x + (ROWS ? 0 : (size_t)r * a.D);
  const int nc = f.n_classes, no = f.n_outputs;
  double s[BOOST_MAX_CLASSES];
#pragma unroll
  for (int c = 0; c < BOOST_MAX_CLASSES; ++c) s[c] = c < no ? f.base[c] : 0.0;
  int k = 0;  // t % no
  for (int t = 0; t < f.n_trees; ++t) {
    int node = f.tree_root[t];
    int4 w;
    for (;;) {  // ends at a leaf: every child index is greater than its parent's (host check)
      const int at = MV_IDX(node, f.n_nodes, CK_BOOST_NODE);
      w = LDS ? s_nodes[at] : gnodes[at];
      const int slot = w.z;
      if (slot < 0) break;
      float v;
      if (ROWS)
        v = slot < a.Dm4 ? xr[slot] : xf[MV_IDX(slot - a.Dm4, a.D, CK_BOOST_SLOT)];
      else
        v = (float)xp[MV_IDX(slot, a.D, CK_BOOST_SLOT)];
      const double thr = __hiloint2double(w.y, w.x);
      node = w.w + ((double)v <= thr ? 0 : 1);  // a NaN goes right
    }
    const double leaf = __hiloint2double(w.y, w.x);
    const int kk = MV_IDX(k, no, CK_BOOST_OUT);
#pragma unroll
    for (int c = 0; c < BOOST_MAX_CLASSES; ++c) s[c] = c == kk ? s[c] + leaf : s[c];
    k = k + 1 == no ? 0 : k + 1;
  }
  double p[BOOST_MAX_CLASSES];
  if (no == 1) {  // the binary log-loss: a sigmoid of the one raw score
    p[1] = 1.0 / (1.0 + det_exp2(-s[0], 0.0));
    p[0] = 1.0 - p[1];
#pragma unroll
    for (int c = 2; c < BOOST_MAX_CLASSES; ++c) p[c] = 0.0;
  } else {
    double m = s[0];
#pragma unroll
    for (int c = 1; c < BOOST_MAX_CLASSES; ++c)
      if (c < nc) m = s[c] > m ? s[c] : m;
    double sum = 0.0;
#pragma unroll
    for (int c = 0; c < BOOST_MAX_CLASSES; ++c) {
      p[c] = c < nc ? det_exp2(s[c] - m, 0.0) : 0.0;
      if (c == 1) sum = p[0] + p[1];  // (e[0] + e[1]) + e[2] + ... in class order
      if (c > 1 && c < nc) sum = sum + p[c];
    }
#pragma unroll
    for (int c = 0; c < BOOST_MAX_CLASSES; ++c) p[c] = p[c] / sum;
  }
  if (ROWS) {
    const int mc = a.min_class[st];
    double f1 = p[0];
#pragma unroll
    for (int c = 1; c < BOOST_MAX_CLASSES; ++c) f1 = mc == c ? p[c] : f1;
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
    for (int c = 0; c < BOOST_MAX_CLASSES; ++c)
      if (c < nc) out[c] = p[c];
  }
}

template <bool ROWS>
static hipError_t launch_boost(const BoostArgs& a, bool lds, hipStream_t stream) {
  if (a.total <= 0) return hipSuccess;
  const DBoost& f = a.f;
  if (f.n_trees <= 0 || f.n_nodes <= 0 || f.n_classes < 2 || f.n_classes > BOOST_MAX_CLASSES ||
      f.n_outputs != (f.n_classes == 2 ? 1 : f.n_classes))
    return hipErrorInvalidValue;
  if (lds) {
    if (!boost_lds_ok(f)) return hipErrorInvalidValue;  // the copy would overrun the LDS
    const dim3 grid((unsigned)((a.total + BOOST_LDS_T - 1) / BOOST_LDS_T));
    MV_LAUNCH((k_boost<ROWS, true>), grid, dim3(BOOST_LDS_T),
              (size_t)f.n_nodes * sizeof(BoostNode), stream, a);
  } else {
    const dim3 grid((unsigned)((a.total + BOOST_T - 1) / BOOST_T));
    MV_LAUNCH((k_boost<ROWS, false>), grid, dim3(BOOST_T), 0, stream, a);
  }
  return hipGetLastError();
}

hipError_t launch_boost_rows(const BoostArgs& a, bool lds, hipStream_t stream) {
  if (!a.xml || !a.xfix || !a.min_class || a.n <= 0) return hipErrorInvalidValue;
  return launch_boost<true>(a, lds, stream);
}

hipError_t launch_boost_predict(const BoostArgs& a, bool lds, hipStream_t stream) {
  return launch_boost<false>(a, lds, stream);
}

MV_DEFINE_TAKE_CHECKS(take_checks_boost)

}  // namespace mv
