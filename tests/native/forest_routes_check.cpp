// Prints mlp_route's kind (csrc/routes.h) for problems with and without trees.  Host-only: no
// GPU, no library load.  Built and run by tests/test_forest_cpu.py, which holds the expected
// lines.
#include <cstdio>

#include "routes.h"
using namespace mv;

static float g_w;  // stands for a packed weight array (the routes only test Wp for NULL)

static DProblem problem(int D, int Dm, bool ident, int n_layers, int hidden, int n_trees) {
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
  p.forest.n_trees = n_trees;
  p.forest.n_classes = n_trees ? 2 : 0;
  return p;
}

int main() {
  const Switches sw{};
  std::printf("lcld forest 100 trees   kind=%d\n", mlp_route(problem(47, 28, false, 0, 0, 100), sw).kind);
  std::printf("botnet forest 1 tree    kind=%d\n", mlp_route(problem(756, 432, true, 0, 0, 1), sw).kind);
  std::printf("no model, zero trees    kind=%d\n", mlp_route(problem(47, 28, false, 0, 0, 0), sw).kind);
  std::printf("lcld 64-32-2, zero trees kind=%d\n", mlp_route(problem(47, 28, false, 3, 64, 0), sw).kind);
  std::printf("botnet 64-64-2, zero trees kind=%d\n", mlp_route(problem(756, 432, true, 3, 64, 0), sw).kind);
  std::printf("botnet hidden 256, zero trees kind=%d\n", mlp_route(problem(756, 432, true, 3, 256, 0), sw).kind);
  std::printf("FOREST_ROWS=%d\n", (int)FOREST_ROWS);
  return 0;
}
