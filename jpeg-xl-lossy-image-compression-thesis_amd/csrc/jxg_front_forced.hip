// jxg_front_forced.hip -- the forced encode's instantiation of front_kernel
// (jxg_encode_forced_rgb8), in a translation unit of its own
// (jxg_front_kernel.h: one instantiation family per unit).
#define JXG_FRONT_NS forced_tu
#include "jxg_front_kernel.h"

namespace jxg {

hipError_t upload_front_tables_forced(const FrontTables& t, hipStream_t s) {
  return forced_tu::upload_front_tables(t, s);
}
void launch_front_forced(const FrontArgs& a, uint32_t tiles_x, uint32_t tiles_y, hipStream_t s) {
  const uint32_t nwg = 8 * ((tiles_x * tiles_y + 7) / 8);  // XCD-aware order (front_kernel)
  hipLaunchKernelGGL((forced_tu::front_kernel<false, true, false>), dim3(nwg, 1, 1),
                     dim3(forced_tu::kThreads), 0, s, make_batch(&a, 1));
}

}  // namespace jxg
