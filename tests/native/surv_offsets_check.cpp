// Prints csrc/survival.h's surv_offsets for (N, R) pairs given as arguments "N R N R ...":
// one line "N R alias total" each, alias = the niching temporaries lie inside the dominance
// bitsets, total = the workspace's LDS bytes at mv_survive's one permutation slot and the
// instance's default threads.  Host-only: no GPU, no library load.  Built and run by
// tests/test_survival_edges_cpu.py.
#include <cstdio>
#include <cstdlib>

#include "survival.h"
using namespace mv;

int main(int argc, char** argv) {
  for (int i = 1; i + 1 < argc; i += 2) {
    const int N = std::atoi(argv[i]), R = std::atoi(argv[i + 1]);
    const SurvOff o = surv_offsets(N, R, 1);
    const int alias = N <= SURV_NLDS && o.count == o.dom;
    std::printf("%d %d %d %u\n", N, R, alias, o.total);
  }
  return 0;
}
