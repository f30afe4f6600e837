// jxg_front_forced.hip -- the forced encode's instantiation of front_kernel
// (jxg_encode_forced_rgb8) in a translation unit of its own,
// so that the search instantiations in jxg_front.hip compile to what they
// compile to without it (the reasons are at the top of that file).
#define JXG_FRONT_FORCED_TU 1
#include "jxg_front.hip"
