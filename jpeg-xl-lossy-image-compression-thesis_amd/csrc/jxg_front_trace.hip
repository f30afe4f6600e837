// jxg_front_trace.hip -- the traced encode's instantiations of front_kernel
// (jxg_encode_traced_rgb8), in a translation unit of their own
// (jxg_front_kernel.h: one instantiation family per unit).
#define JXG_FRONT_NS trace_tu
#include "jxg_front_kernel.h"

namespace jxg {

hipError_t upload_front_tables_trace(const FrontTables& t, hipStream_t s) {
  return trace_tu::upload_front_tables(t, s);
}
void launch_front_trace(const FrontArgs& a, uint32_t tiles_x, uint32_t tiles_y, hipStream_t s) {
  const uint32_t nwg = 8 * ((tiles_x * tiles_y + 7) / 8);  // XCD-aware order (front_kernel)
  const Batch<FrontArgs> b = make_batch(&a, 1);
  if (a.proposals & 1u)
    hipLaunchKernelGGL((trace_tu::front_kernel<true, false, true>), dim3(nwg, 1, 1),
                       dim3(trace_tu::kThreads), 0, s, b);
  else
    hipLaunchKernelGGL((trace_tu::front_kernel<false, false, true>), dim3(nwg, 1, 1),
                       dim3(trace_tu::kThreads), 0, s, b);
}

}  // namespace jxg
