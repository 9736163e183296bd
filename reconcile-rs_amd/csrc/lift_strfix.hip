// lift_strfix.hip -- the launcher of the short-string-key lift with fixed-width values
// (lift_strfix.hpp); the kernels are instantiated per row width in lift_strfix{16,32,64}.hip.
#include "internal.hpp"
#include "lift_strfix.hpp"

namespace rh {

hipError_t launch_lift_str_fixed(int w, int vk, int rk, bool tags, const DevCols &c, uint64_t n, uint8_t *fps,
                                 uint8_t *bsums, hipStream_t st, bool *supported) {
    *supported = str_key_supported(w) && (vk == VAL_UNIT || vk == VAL_U32 || vk == VAL_U64);
    if (!*supported || n == 0) return hipSuccess;
    return w == 16   ? launch_lift_strfix_w16(vk, rk, tags, c, n, fps, bsums, st)
           : w == 32 ? launch_lift_strfix_w32(vk, rk, tags, c, n, fps, bsums, st)
                     : launch_lift_strfix_w64(vk, rk, tags, c, n, fps, bsums, st);
}

}  // namespace rh
