// Prints mlp_route's kind (csrc/routes.h) for problems with a kernel machine set, and for
// problems whose svm fields are zero.  Host-only: no GPU, no library load.  Built and run by
// tests/test_svm_cpu.py, which holds the expected lines.
#include <cstdio>

#include "routes.h"
using namespace mv;

static float g_w;  // stands for a packed weight array (the routes only test Wp for NULL)

static DProblem problem(int D, int Dm, bool ident, int n_layers, int hidden, int forest_trees,
                        int boost_trees, int svm_vec) {
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
  p.boost.n_nodes = boost_trees * 15;
  p.boost.n_classes = boost_trees ? 2 : 0;
  p.boost.n_outputs = boost_trees ? 1 : 0;
  p.svm.n_vec = svm_vec;
  p.svm.n_out = svm_vec ? 1 : 0;
  p.svm.n_classes = svm_vec ? 2 : 0;
  p.svm.D = svm_vec ? D : 0;
  return p;
}

int main() {
  const Switches sw{};
  std::printf("lcld svc 182 vectors     kind=%d\n", mlp_route(problem(47, 28, false, 0, 0, 0, 0, 182), sw).kind);
  std::printf("botnet logreg 1 vector   kind=%d\n", mlp_route(problem(756, 432, true, 0, 0, 0, 0, 1), sw).kind);
  std::printf("lcld svc 22000 vectors   kind=%d\n", mlp_route(problem(47, 28, false, 0, 0, 0, 0, 22000), sw).kind);
  std::printf("forest, zero svm         kind=%d\n", mlp_route(problem(47, 28, false, 0, 0, 100, 0, 0), sw).kind);
  std::printf("boost, zero svm          kind=%d\n", mlp_route(problem(47, 28, false, 0, 0, 0, 100, 0), sw).kind);
  std::printf("no model, zero svm       kind=%d\n", mlp_route(problem(47, 28, false, 0, 0, 0, 0, 0), sw).kind);
  std::printf("lcld 64-32-2, zero svm   kind=%d\n", mlp_route(problem(47, 28, false, 3, 64, 0, 0, 0), sw).kind);
  std::printf("botnet 64-64-2, zero svm kind=%d\n", mlp_route(problem(756, 432, true, 3, 64, 0, 0, 0), sw).kind);
  std::printf("botnet hidden 256, zero svm kind=%d\n", mlp_route(problem(756, 432, true, 3, 256, 0, 0, 0), sw).kind);
  std::printf("SVM_ROWS=%d SVM_VB=%d SVM_FC=%d\n", (int)SVM_ROWS, SVM_VB, SVM_FC);
  return 0;
}
