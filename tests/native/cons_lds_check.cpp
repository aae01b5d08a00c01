// Prints csrc/kernels.h's LDS sizes of the wave-per-row kernels for a constraints-only problem
// over D real features (V = Vr = Dm = D genes, no one-hot group, no ABS_SUMDIFF op), as
// api.cpp build_problem checks them against the CU's 160 KiB: arguments "D C n_pool C n_pool
// ...", one line "C n_pool cons_lds_total gen_lds_total" per pair.  n_pool is the index pool
// with the MV_OP_EXPR bytecode and constants appended.  Host-only: no GPU, no library load.
// Built and run by tests/test_expr_edges_cpu.py, which pins the column count that
// tests/test_gpu_expr.py runs at the bound.
#include <cstdio>
#include <cstdlib>

#include "kernels.h"
using namespace mv;

int main(int argc, char** argv) {
  if (argc < 2) return 1;
  const int D = std::atoi(argv[1]);
  for (int i = 2; i + 1 < argc; i += 2) {
    DProblem p{};
    p.D = D;
    p.V = p.Vr = p.Dm = D;
    p.Dm4 = (D + 15) & ~15;
    p.ident = 1;
    p.full_ops = 2;
    p.C = std::atoi(argv[i]);
    p.n_pool = std::atoi(argv[i + 1]);
    const VaryOff o = vary_offsets(p);
    std::printf("%d %d %u %u\n", p.C, p.n_pool, cons_lds_total(o), gen_lds(o, false, true).total);
  }
  return 0;
}
