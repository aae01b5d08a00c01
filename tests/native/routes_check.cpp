// Prints the route table of csrc/routes.h: which kernel instance row_route / mlp_route pick
// for hand-filled problems, and vary_rows_per_wg's chunking.  Host-only: no GPU, no library
// load.  Built and run by tests/test_routes_cpu.py, which holds the expected lines.
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "kernels.h"
#include "routes.h"
using namespace mv;

static float g_w;  // stands for a packed weight array (the routes only test Wp for NULL)
static int4 g_hdr;
static int g_mw;
static double g_mu;

// A problem as mv_create_problem / mv_set_model fill it (api.cpp): Dm4 is Dm padded to a
// multiple of 16; mlp2 = every hidden width a multiple of 16 and <= 128; Wp packed when every
// hidden width is a multiple of 16; xml_direct = mlp2 && ident.
static DProblem problem(int D, int V, int Dm, int C, bool ident, int full_ops,
                        std::initializer_list<int> hidden_out, bool bf16 = false) {
  DProblem p{};
  p.D = D;
  p.V = p.Vr = V;
  p.Dm = Dm;
  p.Dm4 = (Dm + 15) & ~15;
  p.C = C;
  p.ident = ident;
  p.full_ops = full_ops;
  p.n_layers = (int)hidden_out.size();
  if (p.n_layers) {
    p.dims[0] = D;
    int l = 1;
    for (int h : hidden_out) p.dims[l++] = h;
    p.mlp2 = 1;
    bool pack16 = true;
    for (l = 1; l < p.n_layers; ++l) {
      p.mlp2 &= p.dims[l] % 16 == 0 && p.dims[l] <= 128;
      pack16 &= p.dims[l] % 16 == 0;
    }
    for (l = 0; l + 1 < p.n_layers && pack16; ++l) p.Wp[l] = &g_w;
    p.xml_direct = p.mlp2 && ident;
    p.mlp_bf16 = bf16;
  }
  return p;
}
// botnet: 756 features, 432 mutable = genes (IDENT), 360 constraint ops, slim program
static DProblem botnet(std::initializer_list<int> net, int Dm = 432, bool bf16 = false) {
  DProblem p = problem(756, Dm, Dm, 360, true, 0, net, bf16);
  p.n_sumdiff = 24;
  p.slim = 1;
  return p;
}
// LCLD: 47 features, V genes (one-hot groups: not IDENT), 28 mutable, 10 financial ops
static DProblem lcld(std::initializer_list<int> net, int V = 15, int full_ops = 1) {
  return problem(47, V, 28, 10, false, full_ops, net);
}

// MV_XML, MV_MLP_V1, MV_MLPW: mv_engine_create leaves xml_direct 0 (the row kernels write the
// fp32 ML rows)
static DProblem rows_written(DProblem p) {
  p.xml_direct = 0;
  return p;
}
static void mlp(const char* name, const DProblem& p, const Switches& sw = Switches{}) {
  const MlpRoute r = mlp_route(p, sw);
  std::printf("mlp %-34s kind=%d rw=%d no=%d xml=%d cj=%d bf=%d direct=%d co=%d maxct=%d\n", name,
              r.kind, r.rw, r.no, (int)r.xml, r.cj, (int)r.bf, (int)r.direct, (int)r.co, r.maxct);
}

static RowsArgs rows(const DProblem& p, int mode = 1, int cx_kind = 0, bool plan = true,
                     int do_eval = 1) {
  RowsArgs a{};
  a.p = p;
  a.n = 100;
  a.total = 400;
  a.mode = mode;
  a.cx_kind = cx_kind;
  a.do_eval = do_eval;
  if (plan) {
    a.plan_hdr = &g_hdr;
    a.plan_mw = &g_mw;
    a.plan_mu = &g_mu;
  }
  return a;
}
static void row(const char* name, const RowsArgs& a, const Switches& sw = Switches{}) {
  const RowRoute r = row_route(a, sw);
  std::printf("row %-34s kind=%d nt=%d ident=%d sbx=%d slim=%d cons=%d nv=%d full=%d "
              "need_plan=%d plan_missing=%d\n", name, r.kind, r.nt, (int)r.ident, (int)r.sbx,
              (int)r.slim, r.cons, r.nv, (int)r.full, (int)r.need_plan, (int)r.plan_missing);
}
static void chunk(const char* name, int n, int states, int cus, int cap) {
  const int rw = vary_rows_per_wg(n, states, cus, cap);
  const int per = (n + rw - 1) / rw;
  std::printf("rows_per_wg %-26s rows=%d chunks_per_state=%d workgroups=%d\n", name, rw, per,
              per * (states > 0 ? states : 1));
}

// The synthetic shapes of tests/synth_problem.py (one line per GPU case of
// tests/test_gpu_row_routes.py; "/sbx": the case's second run): the attack's problem as
// build_problem derives it -- stored genes V of Vr, Dm, C, ident, full_ops, n_sumdiff, slim --
// under a D-32-16-2 classifier.  The line names the shape, then gives the row route and the
// classifier kind, so the instance a GPU case claims to reach is pinned here.
struct Synth {
  const char* name;
  int V, Vr, Dm, C, ident, full_ops, n_sd, slim, sbx;
};
static const Synth kSynth[] = {
    {"n8p", 8, 8, 8, 5, 1, 0, 0, 0, 0},
    {"n8p/sbx", 8, 8, 8, 5, 1, 0, 0, 0, 1},
    {"n8f", 8, 8, 13, 8, 0, 1, 0, 0, 0},
    {"n9", 9, 9, 9, 6, 1, 0, 0, 0, 0},
    {"n16f", 16, 16, 19, 10, 0, 1, 0, 0, 0},
    {"n17f", 17, 17, 22, 10, 0, 1, 0, 0, 0},
    {"n32", 32, 32, 64, 64, 0, 0, 0, 0, 0},
    {"n32d", 32, 32, 65, 64, 0, 0, 0, 0, 0},
    {"n32c", 32, 32, 64, 65, 0, 0, 0, 0, 0},
    {"n8s", 8, 8, 8, 6, 1, 0, 1, 0, 0},
    {"n2", 2, 2, 2, 2, 1, 0, 0, 1, 0},
    {"g33", 33, 33, 33, 20, 1, 0, 0, 0, 0},
    {"g33/sbx", 33, 33, 33, 20, 1, 0, 0, 0, 1},
    {"g64", 64, 64, 64, 40, 1, 0, 0, 0, 0},
    {"g65", 65, 65, 65, 40, 1, 0, 0, 0, 0},
    {"g65/sbx", 65, 65, 65, 40, 1, 0, 0, 0, 1},
    {"g128", 128, 128, 128, 70, 1, 0, 0, 0, 0},
    {"o40f", 40, 40, 51, 24, 0, 1, 0, 0, 0},
    {"o100p", 100, 100, 150, 70, 0, 0, 0, 0, 0},
    {"o100p/sbx", 100, 100, 150, 70, 0, 0, 0, 0, 1},
    {"o300f", 300, 300, 330, 100, 0, 1, 0, 0, 0},
    {"o520p", 520, 520, 600, 150, 0, 0, 0, 0, 0},
    {"c129", 129, 129, 129, 70, 1, 0, 0, 1, 0},
    {"c129/sbx", 129, 129, 129, 70, 1, 0, 0, 1, 1},
    {"c256", 256, 256, 256, 100, 1, 0, 0, 1, 0},
    {"c257", 257, 257, 257, 100, 1, 0, 0, 1, 0},
    {"c384", 384, 384, 384, 130, 1, 0, 0, 1, 0},
    {"c384/sbx", 384, 384, 384, 130, 1, 0, 0, 1, 1},
    {"c385", 385, 385, 385, 130, 1, 0, 0, 1, 0},
    {"c512", 512, 512, 512, 150, 1, 0, 0, 1, 0},
    {"c513", 513, 513, 513, 150, 1, 0, 0, 1, 0},
    {"c1024", 1024, 1024, 1024, 300, 1, 0, 0, 1, 0},
    {"c300x", 300, 300, 300, 400, 1, 0, 0, 0, 0},
    {"c300d", 300, 300, 300, 100, 1, 0, 3, 1, 0},
    {"k_slab", 136, 200, 136, 80, 1, 0, 0, 1, 0},
    {"k_last", 199, 200, 199, 80, 1, 0, 0, 1, 0},
    {"k_odd", 143, 200, 143, 80, 1, 0, 0, 1, 0},
    {"k_few", 3, 200, 3, 80, 1, 0, 0, 1, 0},
    {"k_mixed", 160, 200, 160, 80, 1, 0, 0, 1, 0},
    // MV_OP_EXPR columns (full_ops 2): k_gen + k_consx<IDENT, NT> at every vary_nt edge
    {"x64", 64, 64, 64, 40, 1, 2, 0, 0, 0},
    {"x65", 65, 65, 65, 40, 1, 2, 0, 0, 0},
    {"x65/sbx", 65, 65, 65, 40, 1, 2, 0, 0, 1},
    {"x128", 128, 128, 128, 70, 1, 2, 0, 0, 0},
    {"x129", 129, 129, 129, 70, 1, 2, 0, 0, 0},
    {"x256", 256, 256, 256, 100, 1, 2, 0, 0, 0},
    {"x257", 257, 257, 257, 100, 1, 2, 0, 0, 0},
    {"x512", 512, 512, 512, 150, 1, 2, 0, 0, 0},
    {"x513", 513, 513, 513, 150, 1, 2, 0, 0, 0},
    {"x1024", 1024, 1024, 1024, 300, 1, 2, 0, 0, 0},
    {"x300c", 300, 300, 300, 400, 1, 2, 3, 0, 0},
    {"xo32d", 32, 32, 65, 64, 0, 2, 0, 0, 0},
    {"xo100", 100, 100, 150, 70, 0, 2, 0, 0, 0},
    {"xo100/sbx", 100, 100, 150, 70, 0, 2, 0, 0, 1},
    {"xo300f", 300, 300, 330, 100, 0, 2, 0, 0, 0},
    {"xo520", 520, 520, 600, 150, 0, 2, 0, 0, 0},
    {"xn8f", 8, 8, 13, 8, 0, 2, 0, 0, 0},
    {"xk_last", 199, 200, 199, 80, 1, 2, 0, 0, 0},
    {"xk_odd", 143, 200, 143, 80, 1, 2, 0, 0, 0},
    {"xk_few", 3, 200, 3, 80, 1, 2, 0, 0, 0},
    {"xk_mixed", 160, 200, 160, 80, 1, 2, 0, 0, 0},
};
static void synth(const Synth& s) {
  DProblem p = problem(2048, s.V, s.Dm, s.C, s.ident != 0, s.full_ops, {32, 16, 2});
  p.Vr = s.Vr;
  p.compact = s.V < s.Vr;
  p.n_sumdiff = s.n_sd;
  p.slim = s.slim;
  char name[96];
  std::snprintf(name, sizeof name, "synth %s V%d Dm4 %d C%d i%d f%d sd%d c%d s%d x%d", s.name,
                p.V, p.Dm4, p.C, s.ident, s.full_ops, s.n_sd, (int)p.compact, s.slim, s.sbx);
  const RowRoute r = row_route(rows(p, 1, s.sbx), Switches{});
  std::printf("row %-34s kind=%d nt=%d ident=%d sbx=%d slim=%d cons=%d nv=%d full=%d "
              "need_plan=%d plan_missing=%d mlp=%d\n", name, r.kind, r.nt, (int)r.ident,
              (int)r.sbx, (int)r.slim, r.cons, r.nv, (int)r.full, (int)r.need_plan,
              (int)r.plan_missing, mlp_route(p, Switches{}).kind);
}

// The classifier-fallback shapes of tests/synth_problem.py MLP_CASES (IDENT, V = Dm plain
// genes, 12 slim columns) under their own nets, in the fp32 and the bf16 mode and under
// MV_MLP_V1 (m639t: with MV_MLPR=0) where a GPU case sets it: the k_mlp<MAXCT, BF> instance each one names.
static void mlp_synth(const char* name, int Dm, std::initializer_list<int> net, bool bf16 = false,
                      int v1 = 0) {
  DProblem p = problem(Dm + 14, Dm, Dm, 12, true, 0, net, bf16);
  p.slim = 1;
  Switches sw;
  if (v1) {  // MV_MLP_V1: set at create, where it has the fp32 ML rows written (xml_direct 0)
    sw.mlp_v1 = true;
    p.xml_direct = 0;
    sw.mlpr_off = v1 == 2;  // the case also sets MV_MLPR=0
  }
  char nets[64] = "", full[96];
  for (int h : net) std::snprintf(nets + std::strlen(nets), sizeof nets - std::strlen(nets),
                                  "%s%d", nets[0] ? "-" : "", h);
  std::snprintf(full, sizeof full, "synth %s Dm4 %d %s %s%s", name, p.Dm4, nets,
                bf16 ? "bf16" : "fp32", v1 ? " MV_MLP_V1" : "");
  mlp(full, p, sw);
}
// mv_engine_create's LDS check (api.cpp build_problem: mlp_lds_bytes <= 160 KiB) and the two
// wide kernels' own budgets, at both sides of each edge
static void lds(int Dm4, std::initializer_list<int> net) {
  DProblem p = problem(Dm4 + 14, Dm4, Dm4, 12, true, 0, net);
  const int nl = p.n_layers;
  const size_t v1 = mlp_lds_bytes(p.Dm4, max_hidden(p.dims, nl), p.dims[nl - 1], p.dims[nl]);
  std::printf("lds Dm4 %d", Dm4);
  for (int h : net) std::printf("-%d", h);
  std::printf(" k_mlp=%zu create=%s k_mlpw32=%u k_mlpw=%u\n", v1,
              v1 <= 160 * 1024 ? "ok" : "refused", mlpw32_lds(p).total, mlpw_lds(p).total);
}

int main() {
  // --- classifier routes, default switches
  mlp("botnet 312-64-64-32-2", botnet({64, 64, 32, 2}, 312));
  mlp("botnet 312-64-64-32-3", botnet({64, 64, 32, 3}, 312));
  mlp("botnet 432-64-64-32-2", botnet({64, 64, 32, 2}));
  mlp("botnet odd Dm 431-64-32-2", botnet({64, 32, 2}, 431));
  mlp("lcld 64-32-2 (ML rows)", lcld({64, 32, 2}));
  mlp("lcld 64-32-3 (ML rows)", lcld({64, 32, 3}));
  mlp("botnet hidden 80 (genes, even Dm)", botnet({80, 32, 2}));
  mlp("botnet hidden 128 (genes)", botnet({128, 64, 2}));
  mlp("botnet hidden 80 (genes, odd Dm)", botnet({80, 32, 2}, 431));
  mlp("lcld hidden 80 (ML rows)", lcld({80, 32, 2}));
  mlp("lcld hidden 128 (ML rows)", lcld({128, 64, 2}));
  mlp("bf16 hidden 64", botnet({64, 64, 32, 2}, 432, true));
  mlp("bf16 hidden 128", botnet({128, 64, 2}, 432, true));
  mlp("bf16 hidden 256", botnet({256, 128, 2}, 432, true));
  mlp("bf16 hidden 512", botnet({512, 512, 256, 2}, 432, true));
  mlp("fp32 hidden 144", botnet({144, 64, 2}));
  mlp("fp32 hidden 256", botnet({256, 128, 2}));
  mlp("fp32 hidden 512", botnet({512, 512, 256, 2}));
  mlp("fp32 512 wide, 8 classes, Dm4 432", botnet({512, 512, 8}));
  // mlpw32_lds = 256 + head + 64 rows * (max(Dm4, widths) + 4) * 4 B > 160 KiB from Dm4 = 640
  mlp("fp32 hidden 512, Dm4 624", botnet({512, 256, 2}, 624));
  mlp("fp32 hidden 512, Dm4 640", botnet({512, 256, 2}, 640));
  mlp("bf16 hidden 512, Dm4 640", botnet({512, 256, 2}, 640, true));
  // (Dm4 % 16 != 0 cannot occur: Dm4 is Dm rounded up to a multiple of 16 where the problem
  // is created, and nothing else writes it; the guards in mlpr_ok / mlpw32_ok restate that)
  mlp("fp32 hidden 520 (not 16 k)", botnet({520, 64, 2}));
  mlp("fp32 hidden 200 (not 16 k)", botnet({200, 64, 2}));
  mlp("fp32 hidden 528 (> 512)", botnet({528, 64, 2}));
  mlp("fp32 9 classes, hidden 256", botnet({256, 64, 9}));
  mlp("fp32 9 classes, hidden 64", botnet({64, 32, 9}));
  mlp("one Dense layer", botnet({2}));
  mlp("no model", botnet({}));

  // --- classifier switches, each alone
  Switches s;
  s = Switches{}, s.mlpr_off = true;
  mlp("MV_MLPR=0 botnet 312-64-64-32-2", botnet({64, 64, 32, 2}, 312), s);
  mlp("MV_MLPR=0 lcld 64-32-2", lcld({64, 32, 2}), s);
  s = Switches{}, s.mlpr_rw = 2;
  mlp("MV_MLPR_RW=2 botnet 312-64-64-32-2", botnet({64, 64, 32, 2}, 312), s);
  mlp("MV_MLPR_RW=2 botnet ... 3 classes", botnet({64, 64, 32, 3}, 312), s);
  mlp("MV_MLPR_RW=2 lcld 64-32-2", lcld({64, 32, 2}), s);
  s = Switches{}, s.mlpr_rw = 7;
  mlp("MV_MLPR_RW=7 botnet 312-64-64-32-2", botnet({64, 64, 32, 2}, 312), s);
  s = Switches{}, s.mlp_v1 = true;
  mlp("MV_MLP_V1 botnet hidden 128", rows_written(botnet({128, 64, 2})), s);
  mlp("MV_MLP_V1 botnet 312-64-64-32-2", rows_written(botnet({64, 64, 32, 2}, 312)), s);
  mlp("MV_MLP_V1 bf16 hidden 128", rows_written(botnet({128, 64, 2}, 432, true)), s);
  s = Switches{}, s.mlpw = true;
  mlp("MV_MLPW bf16 hidden 64", rows_written(botnet({64, 64, 32, 2}, 432, true)), s);
  mlp("MV_MLPW fp32 hidden 128", rows_written(botnet({128, 64, 2})), s);
  s = Switches{}, s.mlpw_off = true;
  mlp("MV_MLPW_OFF bf16 hidden 256", botnet({256, 128, 2}, 432, true), s);
  mlp("MV_MLPW_OFF bf16 hidden 64", botnet({64, 64, 32, 2}, 432, true), s);
  s = Switches{}, s.mlpw32_off = true;
  mlp("MV_MLPW32=0 fp32 hidden 144", botnet({144, 64, 2}), s);
  mlp("MV_MLPW32=0 fp32 hidden 512", botnet({512, 512, 256, 2}), s);
  s = Switches{}, s.mlp_co_off = true;
  mlp("MV_MLP_CO=0 botnet hidden 80", botnet({80, 32, 2}), s);

  // --- the k_mlp fallback's cases and their LDS edges (160 KiB = 163840)
  mlp_synth("m608w", 608, {512, 512, 2});
  mlp_synth("m609w", 609, {512, 512, 2});
  mlp_synth("m609w", 609, {512, 512, 2}, true);
  mlp_synth("m736w", 736, {512, 272, 3});
  mlp_synth("m1008w", 1008, {144, 240, 3});
  mlp_synth("m1008w", 1008, {144, 240, 3}, true);
  mlp_synth("m640n", 640, {48, 80, 2});
  mlp_synth("m640n", 640, {48, 80, 2}, false, 1);
  mlp_synth("m639t", 639, {32, 16, 8});
  mlp_synth("m639t", 639, {32, 16, 8}, false, 2);
  mlp("MV_MLP_V1 even Dm 640-32-16-8",
      rows_written(problem(654, 640, 640, 12, true, 0, {32, 16, 8})),
      [] { Switches t; t.mlp_v1 = true; return t; }());
  mlp("bf16 botnet 756-512-512-8", botnet({512, 512, 8}, 432, true));
  mlp("bf16 botnet 756-512-256-8", botnet({512, 256, 8}, 432, true));
  lds(608, {512, 512, 2});
  lds(624, {512, 512, 2});
  lds(720, {512, 512, 2});
  lds(736, {512, 512, 2});
  lds(736, {512, 272, 3});
  lds(752, {512, 272, 3});
  lds(1008, {144, 240, 3});
  lds(1024, {144, 240, 3});
  lds(432, {512, 512, 8});
  lds(432, {512, 256, 8});

  // --- row routes
  const std::initializer_list<int> net = {64, 64, 32, 2};
  row("botnet full layout V 432", rows(botnet(net)));
  DProblem compact = botnet(net, 312);
  compact.Vr = 432;
  compact.compact = 1;
  row("botnet compact V 312 Vr 432", rows(compact));
  row("botnet SBX", rows(botnet(net), 1, 1));
  DProblem fat = botnet(net);
  fat.slim = 0;
  row("botnet slim 0", rows(fat));
  row("botnet slim 0 SBX", rows(fat, 1, 1));
  row("botnet mode 0 (genes given)", rows(botnet(net), 0, 0, false));
  row("botnet mode 1 without a plan", rows(botnet(net), 1, 0, false));
  row("botnet do_eval 0", rows(botnet(net), 1, 0, true, 0));
  row("lcld V 8", rows(lcld(net, 8)));
  row("lcld V 9", rows(lcld(net, 9)));
  row("lcld V 15", rows(lcld(net, 15)));
  row("lcld V 16", rows(lcld(net, 16)));
  row("lcld V 17", rows(lcld(net, 17)));
  row("lcld V 32", rows(lcld(net, 32)));
  row("lcld V 33", rows(lcld(net, 33)));
  row("lcld V 15 without financial ops", rows(lcld(net, 15, 0)));
  row("lcld SBX", rows(lcld(net), 1, 1));
  row("lcld SBX, mode 0", rows(lcld(net), 0, 1));
  row("lcld expr columns (full_ops 2)", rows(lcld(net, 15, 2)));
  DProblem bx = botnet(net);
  bx.full_ops = 2;
  bx.slim = 0;
  row("botnet expr columns (full_ops 2)", rows(bx));
  DProblem lc = lcld(net);
  lc.compact = 1;
  row("lcld compact", rows(lc));
  DProblem lsd = lcld(net);
  lsd.n_sumdiff = 1;
  row("lcld with a sum-diff op", rows(lsd));
  DProblem lwide = lcld(net);
  lwide.C = 65;
  row("lcld 65 ops", rows(lwide));
  row("lcld do_eval 0", rows(lcld(net), 1, 0, true, 0));
  // IDENT, no model-side effect: max(V, Dm4) at k_genc's threshold
  row("ident max(V, Dm4) 128", rows(problem(200, 128, 128, 40, true, 0, net)));
  row("ident max(V, Dm4) 129", rows(problem(200, 129, 129, 40, true, 0, net)));
  row("ident V 120 (Dm4 128)", rows(problem(200, 120, 120, 40, true, 0, net)));
  row("ident V 40 (one gene per lane)", rows(problem(200, 40, 40, 70, true, 0, net)));
  row("ident V 100 (two per lane)", rows(problem(200, 100, 100, 70, true, 0, net)));
  row("ident V 257 (k_genc NT 5)", rows(problem(400, 257, 257, 70, true, 0, net)));
  row("ident V 384 (k_genc NT 6)", rows(problem(400, 384, 384, 70, true, 0, net)));
  row("ident V 512 (k_genc NT 8)", rows(problem(600, 512, 512, 70, true, 0, net)));
  row("ident V 513 (k_genc NT 16)", rows(problem(600, 513, 513, 70, true, 0, net)));
  row("not ident V 432", rows(problem(756, 432, 400, 360, false, 0, net)));
  row("not ident V 600", rows(problem(756, 600, 400, 360, false, 0, net)));
  s = Switches{}, s.narrow_off = true;
  row("MV_NARROW=0 lcld V 15", rows(lcld(net, 15)), s);
  row("MV_NARROW=0 botnet", rows(botnet(net)), s);
  s = Switches{}, s.genc_off = true;
  row("MV_GENC=0 botnet", rows(botnet(net)), s);
  row("MV_GENC=0 botnet SBX", rows(botnet(net), 1, 1), s);
  row("MV_GENC=0 lcld V 15", rows(lcld(net, 15)), s);

  // --- rows per workgroup
  chunk("n 100, 387 states", 100, 387, 256, 0);
  chunk("n 203, 387 states", 203, 387, 256, 0);
  chunk("n 100, 48 states", 100, 48, 256, 0);
  chunk("n 100, 12 states", 100, 12, 256, 0);
  chunk("n 100, 1 state", 100, 1, 256, 0);
  chunk("n 3, 387 states", 3, 387, 256, 0);
  chunk("n 3, 1 state", 3, 1, 256, 0);
  chunk("n 100, states unknown", 100, 0, 256, 0);
  chunk("n 100, 48 states, 304 CUs", 100, 48, 304, 0);
  chunk("n 100, 48 states, cap 16", 100, 48, 256, 16);
  chunk("n 100, 387 states, cap 64", 100, 387, 256, 64);
  chunk("n 100, 387 states, cap 1", 100, 387, 256, 1);

  // --- the synthetic shapes of the GPU row-route cases
  for (const Synth& s : kSynth) synth(s);
  return 0;
}
