// jxg_front_trace.hip -- the traced encode's instantiations of front_kernel
// (jxg_encode_traced_rgb8) in a translation unit of its own,
// as the forced encode's (jxg_front_forced.hip): the search instantiations in
// jxg_front.hip compile to what they compile to without it.
#define JXG_FRONT_TRACE_TU 1
#include "jxg_front.hip"
