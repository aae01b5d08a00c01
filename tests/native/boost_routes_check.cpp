// Prints mlp_route's kind (csrc/routes.h) for problems with a boosted ensemble on either side of
// k_boost's LDS budget, and for problems whose boost fields are zero.  Host-only: no GPU, no
// library load.  Built and run by tests/test_boost_cpu.py, which holds the expected lines.
#include <cstdio>

#include "routes.h"
using namespace mv;

static float g_w;  // stands for a packed weight array (the routes only test Wp for NULL)

static DProblem problem(int D, int Dm, bool ident, int n_layers, int hidden, int forest_trees,
                        int boost_trees, int boost_nodes, int classes = 2) {
  DProblem p{};
  p.D = D;
  p.V = p.Vr = Dm;
  p.Dm = Dm;
  p.Dm4 = (Dm + 15) & ~15;
  p.ident = ident;
  p.n_layers = n_layers;
  if (n_layers) {
    p.dims[0] = D;
    for (int l = 1; l < n_layers; ++l) p.dims[l] = hidden;
    p.dims[n_layers] = 2;
    p.mlp2 = hidden % 16 == 0 && hidden <= 128;
    for (int l = 0; l + 1 < n_layers; ++l) p.Wp[l] = &g_w;
    p.xml_direct = p.mlp2 && ident;
  }
  p.forest.n_trees = forest_trees;
  p.forest.n_classes = forest_trees ? 2 : 0;
  p.boost.n_trees = boost_trees;
  p.boost.n_nodes = boost_nodes;
  p.boost.n_classes = boost_trees ? classes : 0;
  p.boost.n_outputs = boost_trees ? (classes == 2 ? 1 : classes) : 0;
  return p;
}

int main() {
  const Switches sw{};
  Switches off{};
  off.boost_lds_off = true;
  const int fit = BOOST_LDS_MAX_BYTES / (int)sizeof(BoostNode);  // nodes that fill the budget
  std::printf("lcld boost 100 x depth 3 kind=%d\n", mlp_route(problem(47, 28, false, 0, 0, 0, 100, 1500), sw).kind);
  std::printf("botnet boost 1 node      kind=%d\n", mlp_route(problem(756, 432, true, 0, 0, 0, 1, 1), sw).kind);
  std::printf("boost at the budget      kind=%d\n", mlp_route(problem(47, 28, false, 0, 0, 0, 300, fit, 3), sw).kind);
  std::printf("boost one node over      kind=%d\n", mlp_route(problem(47, 28, false, 0, 0, 0, 300, fit + 1, 3), sw).kind);
  std::printf("boost 1.6 M nodes        kind=%d\n", mlp_route(problem(47, 28, false, 0, 0, 0, 800, 1600000, 8), sw).kind);
  std::printf("lds switched off         kind=%d\n", mlp_route(problem(47, 28, false, 0, 0, 0, 100, 1500), off).kind);
  std::printf("forest, zero boost       kind=%d\n", mlp_route(problem(47, 28, false, 0, 0, 100, 0, 0), sw).kind);
  std::printf("no model, zero boost     kind=%d\n", mlp_route(problem(47, 28, false, 0, 0, 0, 0, 0), sw).kind);
  std::printf("lcld 64-32-2, zero boost kind=%d\n", mlp_route(problem(47, 28, false, 3, 64, 0, 0, 0), sw).kind);
  std::printf("botnet 64-64-2, zero boost kind=%d\n", mlp_route(problem(756, 432, true, 3, 64, 0, 0, 0), sw).kind);
  std::printf("botnet hidden 256, zero boost kind=%d\n", mlp_route(problem(756, 432, true, 3, 256, 0, 0, 0), sw).kind);
  std::printf("lds switched off, zero boost kind=%d\n", mlp_route(problem(756, 432, true, 3, 64, 0, 0, 0), off).kind);
  std::printf("FOREST_ROWS=%d BOOST_ROWS=%d BOOST_ROWS_LDS=%d budget_nodes=%d\n", (int)FOREST_ROWS,
              (int)BOOST_ROWS, (int)BOOST_ROWS_LDS, fit);
  return 0;
}
