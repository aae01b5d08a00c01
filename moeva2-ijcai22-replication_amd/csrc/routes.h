// Which kernel instance a launch runs: the one place where the row kernels' and the
// classifier's routes are decided.  launch_gen / launch_cons / launch_mlp (eval.hip) switch
// on the route, row_kernel_kind / mlp_kernel_kind report its kind.  Host-only logic over the
// DProblem / RowsArgs fields and the kernels' LDS-size helpers below: no HIP call, no
// getenv -- the caller fills Switches and passes the CU count, so the table is checked
// without a GPU (tests/native/routes_check.cpp).  A new route is added here.
#pragma once
#include "engine.h"

namespace mv {

// --- shapes the kernels take (shared with the kernels themselves) ------------------------

__host__ __device__ inline int max_hidden(const int* dims, int n_layers) {
  int h = 16;
  for (int l = 1; l < n_layers; ++l) h = dims[l] > h ? dims[l] : h;
  return h;
}

// k_mlp / k_predict MAXCT: 16-column tiles per wave over the widest hidden layer
inline int mlp_maxct(int hmax) {
  const int nct = hmax / 16;
  return nct <= 4 ? 1 : nct <= 8 ? 2 : nct <= 16 ? 4 : 8;
}

__host__ __device__ inline int mlp2_hmax(const DProblem& p) {
  int h = 16;
  for (int l = 1; l < p.n_layers; ++l) h = p.dims[l] > h ? p.dims[l] : h;
  return h;
}

constexpr int NARROW_MAXV = 32;  // genes per row held in registers
constexpr int NARROW_MAXF = 64;  // mutable features (Dm4) and constraint ops
__host__ __device__ inline bool narrow_ok(const DProblem& p) {
  return p.V <= NARROW_MAXV && p.Dm4 <= NARROW_MAXF && p.C <= NARROW_MAXF &&
         p.n_sumdiff == 0 && p.Dm >= 1;
}

// k_mlpr LDS: the ML scaler at the mutable features (mlS, mlM), the final Dense layer, the
// hidden layers' packed weights and biases (read per tile: from L2 each hidden layer waited
// out a ~3 k-cycle round trip, MV_MLP_PHASES "hidden" 16.9 k cycles per tile), then per wave
// its tile's bias1 rows (landed by LDS DMA while layer 0 runs) and its last-hidden-layer rows.
struct MlprLds {
  unsigned wl, hw, hb, b1, hs, wst, total;
  int hld;  // fp32 row stride of a wave's last-hidden-layer rows
};
__host__ __device__ inline MlprLds mlpr_lds(const DProblem& p, int rw) {
  const int nl = p.n_layers;
  MlprLds L{};
  L.wl = (unsigned)p.Dm4 * 16;  // mlS, mlM
  L.hld = p.dims[nl - 1] + 4;
  L.hw = L.wl + (((unsigned)(p.dims[nl - 1] * p.dims[nl] + p.dims[nl]) * 4 + 15) & ~15u);
  unsigned w = 0, b = 0;
  for (int l = 1; l + 1 < nl; ++l) {
    w += (unsigned)(p.dims[l] * p.dims[l + 1]);
    b += (unsigned)p.dims[l + 1];
  }
  L.hb = L.hw + w * 4;
  // a wave's bias1 rows are in registers before its last-hidden-layer rows are written: one
  // per-wave region serves both
  L.b1 = L.hb + ((b * 4 + 15) & ~15u);
  L.hs = L.b1;
  L.wst = (unsigned)rw * 4 * 1024;
  const unsigned hsz = (unsigned)(rw * 16 * L.hld) * 4;
  L.wst = L.wst > hsz ? L.wst : hsz;
  L.total = L.b1 + 4u * L.wst;
  return L;
}
// The shapes k_mlpr takes: IDENT gene rows (xml_direct) of an even gene count (16-B aligned
// gene pairs), fp32, every MFMA layer's width a multiple of 16 and at most 64, K0 a multiple
// of 16, at most 8 classes.
__host__ __device__ inline bool mlpr_ok(const DProblem& p) {
  // the fp32 ML-row path (LCLD: k_narrow's xml rows, zero-padded to Dm4) takes the XML
  // instance: the same tiles with the rows' fp32 values as layer 0's operands
  if (p.mlp_bf16 || !p.mlp2 || p.n_layers < 2 || (p.xml_direct && ((p.Dm & 1) || p.Dm < 2)))
    return false;
  for (int l = 0; l + 1 < p.n_layers; ++l)
    if (!p.Wp[l]) return false;
  for (int l = 1; l < p.n_layers; ++l)
    if (p.dims[l] % 16 || p.dims[l] > 64) return false;
  return p.Dm4 % 16 == 0 && p.dims[p.n_layers] <= 8 && mlpr_lds(p, 2).total <= 96 * 1024;
}

// k_mlpw / k_mlpw32: 64-row persistent tiles, 8 waves
constexpr int MW_ROWS = 64;
constexpr int MW_T = 512;
struct MwLds {
  unsigned h0, h1, part, total;
  int hs;  // bf16 row stride of the activation buffers
};
__host__ __device__ inline MwLds mlpw_lds(const DProblem& p) {
  const int nl = p.n_layers;
  int w = (p.Dm4 + 31) & ~31;
  for (int l = 1; l < nl; ++l) w = p.dims[l] > w ? p.dims[l] : w;
  MwLds L{};
  L.hs = w + 8;  // 16-B row padding: consecutive rows start 4 banks apart
  const unsigned head =
      256 + (((unsigned)(p.dims[nl - 1] * p.dims[nl] + p.dims[nl]) * 4 + 15) & ~15u);
  const unsigned hb = (unsigned)MW_ROWS * L.hs * 2;
  L.h0 = head;
  L.h1 = L.h0 + hb;
  L.part = L.h1 + hb;
  L.total = L.part + (unsigned)(MW_T / 64) * MW_ROWS * p.dims[nl] * 4;
  return L;
}

struct Mw32Lds {
  unsigned h, part, total;
  int hs;  // fp32 row stride of the activation buffer
};
__host__ __device__ inline Mw32Lds mlpw32_lds(const DProblem& p) {
  const int nl = p.n_layers;
  int w = p.Dm4;
  for (int l = 1; l < nl; ++l) w = p.dims[l] > w ? p.dims[l] : w;
  Mw32Lds L{};
  L.hs = w + 4;  // 16-B row padding: consecutive rows start 4 banks apart
  const unsigned head =
      256 + (((unsigned)(p.dims[nl - 1] * p.dims[nl] + p.dims[nl]) * 4 + 15) & ~15u);
  L.h = head;
  // the wave partials of the final Dense alias the activation buffer: they are written after
  // the barrier that retires the last MFMA layer's reads of it, and that layer's outputs stay
  // in registers (a separate region put 512-wide nets of 8 classes past the CU's LDS and onto
  // the 32-row-tile k_mlp)
  L.part = L.h;
  const unsigned hb = (unsigned)MW_ROWS * L.hs * 4;
  const unsigned pb = (unsigned)(MW_T / 64) * MW_ROWS * p.dims[nl] * 4;
  L.total = L.h + (hb > pb ? hb : pb);
  return L;
}
// The shapes k_mlpw32 takes: every MFMA layer's K and N multiples of 16 (Wp packed), at
// most 4 column tiles per wave (N <= 512: the 256-VGPR budget of two waves per SIMD), LDS
// within the CU's 160 KiB.
__host__ __device__ inline bool mlpw32_ok(const DProblem& p) {
  if (p.n_layers < 2 || !p.Wp[0]) return false;
  for (int l = 1; l < p.n_layers; ++l)
    if (p.dims[l] % 16 || p.dims[l] > 512) return false;
  return p.Dm4 % 16 == 0 && p.dims[p.n_layers] <= 8 && mlpw32_lds(p).total <= 160 * 1024;
}

// --- development switches ----------------------------------------------------------------
// The values of the environment switches, read by the caller (eval.hip read_switches: the
// only getenv of each name).  All false / 1 = the product routes.
struct Switches {
  bool narrow_off = false;  // MV_NARROW=0: keep the wave-per-row kernels (read per launch)
  bool genc_off = false;    // MV_GENC=0: k_gen + k_cons as two launches (read per launch)
  bool mlpr_off = false;    // MV_MLPR=0
  int mlpr_rw = 1;          // MV_MLPR_RW: k_mlpr's 16-row blocks per wave tile, 1 or 2
  bool mlp_v1 = false;      // MV_MLP_V1 set: no k_mlp2
  bool mlpw = false;        // MV_MLPW set: the bf16 mode runs k_mlpw for narrow nets too
  bool mlpw_off = false;    // MV_MLPW_OFF set: no k_mlpw
  bool mlpw32_off = false;  // MV_MLPW32=0: keep the 32-row-tile k_mlp
  bool mlp_co_off = false;  // MV_MLP_CO=0: k_mlp2 without the lane-contiguous gene staging
  bool boost_lds_off = false;  // MV_BOOST_LDS=0: k_boost reads its nodes from L2 (read per launch)
};

// --- row kernels -------------------------------------------------------------------------

// Genes per lane of k_gen / k_cons
inline int vary_nt(const DProblem& p) {
  const int m = p.V > p.Dm4 ? p.V : p.Dm4;
  const int nt = (m + 63) / 64;
  return nt <= 1 ? 1 : nt <= 2 ? 2 : nt <= 4 ? 4 : nt <= 8 ? 8 : 16;
}
// k_genc's genes per lane: the exact ceil(max(V, Dm4) / 64) from 4 to 8 (every unused
// register slot costs a masked instruction per row in every phase), else 16.
__host__ __device__ inline int genc_nt(const DProblem& p) {
  const int m = p.V > p.Dm4 ? p.V : p.Dm4;
  const int nt = (m + 63) / 64;
  return nt <= 4 ? 4 : nt <= 8 ? nt : 16;
}

enum RowKind { ROW_GEN_CONS = 0, ROW_NARROW = 1, ROW_GENC = 2 };
// launch_cons's kernel: none (k_narrow / k_genc did it, or a variation-only launch), k_cons
// with the botnet ops, k_cons with the LCLD financial ops, k_consx (MV_OP_EXPR columns)
enum ConsKind { CONS_NONE = 0, CONS_PLAIN = 1, CONS_FULL = 2, CONS_EXPR = 3 };
struct RowRoute {
  int kind;           // RowKind
  int nt;             // k_gen / k_cons: vary_nt; k_genc: genc_nt; k_narrow: 0
  bool ident;         // k_gen / k_consx / k_cons<false> IDENT (k_genc: always)
  bool sbx;           // k_gen / k_genc SBX
  bool slim;          // k_genc SLIM
  int cons;           // ConsKind
  int nv;             // k_narrow NV (8 / 16 / 32), else 0
  bool full;          // k_narrow FULL
  bool need_plan;     // k_genc in mode 1 takes its draws from the variation plan ...
  bool plan_missing;  // ... and these rows carry none: the launch is hipErrorInvalidValue
};

inline RowRoute row_route(const RowsArgs& a, const Switches& sw) {
  RowRoute r{};
  r.sbx = a.mode == 1 && a.cx_kind == 1;
  // Narrow rows (LCLD-shaped problems): k_narrow does k_gen's and k_cons's work in one launch
  // (two-point crossover; the SBX option and variation-only launches keep the wave-per-row
  // kernels).
  const bool narrow =
      !sw.narrow_off && a.do_eval && narrow_ok(a.p) && !(a.mode == 1 && a.cx_kind == 1) &&
      !a.p.compact &&      // the compact layout runs on the wave-per-row kernels only
      a.p.full_ops != 2;   // and so do MV_OP_EXPR columns (k_gen + k_consx)
  if (narrow) {
    r.kind = ROW_NARROW;
    r.sbx = false;
    r.nv = a.p.V <= 8 ? 8 : a.p.V <= 16 ? 16 : 32;
    r.full = a.p.full_ops != 0;
    return r;
  }
  // k_genc (k_gen + k_cons in one launch) for the wave-per-row evaluation of IDENT problems
  // without the LCLD financial ops (the botnet shape).
  const bool genc = !sw.genc_off && a.do_eval && a.p.ident && !a.p.full_ops &&
                    (a.p.V > a.p.Dm4 ? a.p.V : a.p.Dm4) > 128;
  if (genc) {
    r.kind = ROW_GENC;
    r.nt = genc_nt(a.p);
    r.ident = true;
    r.slim = a.p.slim != 0;
    // k_genc takes mode 1's draws from the variation plan (mv_attack_run's k_survive)
    r.need_plan = a.mode == 1;
    r.plan_missing = r.need_plan && !(a.plan_hdr && a.plan_mw && a.plan_mu);
    return r;
  }
  r.kind = ROW_GEN_CONS;
  r.nt = vary_nt(a.p);
  r.ident = a.p.ident != 0;
  if (!a.do_eval) {
    r.cons = CONS_NONE;
  } else if (a.p.full_ops == 2) {  // MV_OP_EXPR columns: the interpreter instances
    r.cons = CONS_EXPR;
  } else if (a.p.full_ops) {  // LCLD programs: one-hot genes, few genes (k_cons<true, false>)
    r.cons = CONS_FULL;
  } else {
    r.cons = CONS_PLAIN;
  }
  return r;
}

// Rows per k_gen / k_cons workgroup: chunks of at most VARY_ROWS_MAX rows of one state.
// Among the chunk counts from ceil(n / cap) up, the one whose chunks split evenly over the
// workgroup's waves (least idle wave-row slots) -- O = 100 gives 5 chunks of 20 rows, 5 per
// wave, instead of 4 x 25 (waves of 7 and 6 rows): +1.4 % botnet evals/s, +3.3 % with one
// group.  cap_override > 0 (MV_VARY_ROWS, development sweeps) replaces the cap and turns
// both refinements off.
// Small attacks (states_all x chunks below four workgroups per CU, k_genc's occupancy): the
// chunks shrink -- down to one row per wave -- until the row launches fill the chip.  Each
// chunk repeats the workgroup prologue, but with few states the CUs would idle instead, and a
// generation's row-kernel latency is one chunk's (e.g. 48 botnet states, 8-GPU strong scaling
// of configs[1]: 240 workgroups of 20 rows -> 960 of 5 on 256 CUs, 1,200 of 4 on 304).
// Results do not depend on the chunking (every draw is keyed by the row inside its state).
inline int vary_rows_per_wg(int n, int states_all, int cus, int cap_override) {
  // row_draws maps a wave's rows onto lanes 4 k + q, plan_draws onto PLAN_MUT k + q: at
  // most 64 / PLAN_MUT rows per wave
  constexpr int hi = (64 / PLAN_MUT) * VARY_W < 64 ? (64 / PLAN_MUT) * VARY_W : 64;
  const int v = cap_override > 0 ? cap_override : VARY_ROWS_MAX;
  const int cap = v < 4 ? 4 : (v > hi ? hi : v);
  const int c0 = (n + cap - 1) / cap;
  if (cap_override > 0) return (n + c0 - 1) / c0;
  int best = (n + c0 - 1) / c0, waste = INT32_MAX;
  for (int c = c0; c <= c0 + 3; ++c) {
    const int r = (n + c - 1) / c;
    const int w = c * VARY_W * ((r + VARY_W - 1) / VARY_W) - n;
    if (w < waste) {
      waste = w;
      best = r;
    }
  }
  if (states_all <= 0) return best;
  const int target = 4 * cus;
  if ((long long)states_all * ((n + best - 1) / best) >= target) return best;
  const int c = (target + states_all - 1) / states_all;  // chunks per state wanted
  const int r = (n + c - 1) / c;
  return r < VARY_W ? (best < VARY_W ? best : VARY_W) : (r < best ? r : best);
}

// --- classifier --------------------------------------------------------------------------

// mv_get_mlp_kernel's kinds
enum MlpKind {
  MLP_NONE = -1,    // no model: f1 comes from the host
  MLP_V1 = 0,       // k_mlp: 32-row tiles of the fp32 ML rows
  MLP2_GENES = 1,   // k_mlp2 reading the genes (xml_direct)
  MLP2_ROWS = 2,    // k_mlp2 reading the fp32 ML rows
  MLPW = 4,         // k_mlpw (bf16, wide)
  MLPW32 = 5,       // k_mlpw32 (fp32, wide)
  MLPR_GENES = 6,   // k_mlpr reading the genes (hidden widths <= 64)
  MLPR_ROWS = 7,    // k_mlpr reading the fp32 ML rows (XML instance)
  FOREST_ROWS = 8,  // k_forest (a tree ensemble) reading the fp32 ML rows and xfix
  BOOST_ROWS = 9,   // k_boost (a boosted ensemble), the nodes read from global memory (L2)
  BOOST_ROWS_LDS = 10,  // k_boost walking a per-workgroup LDS copy of the nodes (boost_lds_ok)
  SVM_ROWS = 11,    // k_svm (a kernel machine or logistic regression) over the same rows
};
struct MlpRoute {
  int kind;     // MlpKind
  int rw, no;   // k_mlpr RW (1 / 2), NO (2 / 8)
  bool xml;     // k_mlpr XML
  int cj;       // k_mlp2 (1 / 2), k_mlpw / k_mlpw32 (1 / 2 / 4) column tiles per wave
  bool bf;      // k_mlp2 / k_mlp BF
  bool direct;  // k_mlp2 DIRECT
  bool co;      // k_mlp2 CO
  int maxct;    // k_mlp MAXCT (1 / 2 / 4 / 8)
};

inline MlpRoute mlp_route(const DProblem& p, const Switches& sw) {
  MlpRoute r{};
  if (p.forest.n_trees > 0) {  // the problem carries trees (mv_engine_set_forest: no MLP then)
    r.kind = FOREST_ROWS;
    return r;
  }
  if (p.boost.n_trees > 0) {  // mv_engine_set_boost: no MLP and no forest then
    r.kind = !sw.boost_lds_off && boost_lds_ok(p.boost) ? BOOST_ROWS_LDS : BOOST_ROWS;
    return r;
  }
  if (p.svm.n_vec > 0) {  // mv_engine_set_svm: no MLP and no tree ensemble then
    r.kind = SVM_ROWS;
    return r;
  }
  if (p.n_layers == 0) {
    r.kind = MLP_NONE;
    return r;
  }
  if (!sw.mlpr_off && mlpr_ok(p)) {
    r.xml = !p.xml_direct;  // the fp32 ML rows (LCLD)
    r.kind = r.xml ? MLPR_ROWS : MLPR_GENES;
    r.rw = r.xml ? 1 : (sw.mlpr_rw == 1 ? 1 : 2);
    r.no = p.dims[p.n_layers] <= 2 ? 2 : 8;
    return r;
  }
  // (MV_MLPW=1: the bf16 mode runs k_mlpw for narrow nets too -- development A/B)
  if (p.mlp2 && !sw.mlp_v1 && !(p.mlp_bf16 && sw.mlpw)) {
    r.kind = p.xml_direct ? MLP2_GENES : MLP2_ROWS;
    r.cj = mlp2_hmax(p) <= 64 ? 1 : 2;
    r.bf = p.mlp_bf16 != 0;
    r.direct = p.xml_direct != 0;
    // CO: the fp32 path's lane-contiguous gene staging (rows of an even gene count start
    // 16-B aligned in the pool); MV_MLP_CO=0 turns it off (A/B)
    r.co = p.xml_direct && !r.bf && !sw.mlp_co_off && (p.Dm & 1) == 0;
    return r;
  }
  if (p.mlp_bf16 && mlpw_lds(p).total <= 160 * 1024 && !sw.mlpw_off) {
    const int hm = max_hidden(p.dims, p.n_layers);
    r.kind = MLPW;
    r.cj = hm <= 128 ? 1 : hm <= 256 ? 2 : 4;
    return r;
  }
  // fp32 wide classifiers (hidden widths above k_mlp2's 128) on k_mlpw32; MV_MLPW32=0 keeps
  // the 32-row-tile k_mlp (A/B)
  if (!sw.mlpw32_off && !p.mlp_bf16 && mlpw32_ok(p)) {
    const int hm = max_hidden(p.dims, p.n_layers);
    r.kind = MLPW32;
    r.cj = hm <= 128 ? 1 : hm <= 256 ? 2 : 4;
    return r;
  }
  r.kind = MLP_V1;
  r.maxct = mlp_maxct(max_hidden(p.dims, p.n_layers));
  r.bf = p.mlp_bf16 != 0;
  return r;
}

}  // namespace mv
