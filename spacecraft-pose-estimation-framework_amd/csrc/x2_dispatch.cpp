// fp16x2 / fp16mx inverted-residual blocks: from the plan (x2_plan.hpp) to the kernel family that holds its row.
#include "spef_kernels.hpp"

namespace spef {

bool x2_irb_supported(int cin, int hid, int cout, int stride, bool expand, bool res) {
  // (a 1 x 1 map without scratch: the primary table's row, whatever the device)
  return x2_irb_plan({cin, hid, cout, stride, expand, res}, 1, 1, 1, false, 0, 1).known;
}

const char* x2_irb_kernel_name(int cin, int hid, int cout, int stride, bool expand, bool res, int B, int OH, int OW,
                               bool scratch, int io, int num_cu) {
  return x2_irb_plan({cin, hid, cout, stride, expand, res}, B, OH, OW, scratch, io, num_cu).kernel_name();
}

hipError_t launch_x2_irb(const X2Block& b, const X2Plan& p, const X2Args& a, hipStream_t s) {
  if (!a.x || !a.y || !a.wd || !a.bd || !a.wp || !a.bp || (b.expand && (!a.we || !a.be)) || a.io < 0 || a.io > 3)
    return hipErrorInvalidValue;
  if (!p.found) return hipErrorNotSupported;
  return p.kind == 0 ? launch_x2_slab(b, p, a, s) : p.kind >= 5 ? launch_x2_stage3(b, p, a, s) : launch_x2_split(b, p, a, s);
}

}  // namespace spef
