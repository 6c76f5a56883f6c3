// Host program around csrc/x2_plan.hpp alone (no HIP, no library): reads grid points from standard input, one per line
//   cin hid cout stride expand res B OH OW scratch io num_cu
// and prints the plan of each as
//   known found kind TH TW NW WCO P name        (name "-" when no kernel runs)
// tests/test_x2_plan.py builds it with the host compiler and compares the output with tests/golden/x2_kernel_names.json.
#include <cstdio>

#include "x2_plan.hpp"

int main() {
  int cin, hid, cout, st, ex, rs, B, OH, OW, scratch, io, cu;
  while (scanf("%d %d %d %d %d %d %d %d %d %d %d %d", &cin, &hid, &cout, &st, &ex, &rs, &B, &OH, &OW, &scratch, &io,
               &cu) == 12) {
    const spef::X2Plan p = spef::x2_irb_plan({cin, hid, cout, st, ex != 0, rs != 0}, B, OH, OW, scratch != 0, io, cu);
    const char* name = p.kernel_name();
    printf("%d %d %d %d %d %d %d %d %s\n", (int)p.known, (int)p.found, p.kind, p.TH, p.TW, p.NW, p.WCO, p.P,
           name ? name : "-");
  }
  return 0;
}
