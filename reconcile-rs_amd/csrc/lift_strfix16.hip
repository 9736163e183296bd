// lift_strfix16.hip -- lift_strfix.hpp instantiated for 16-byte key rows.
#include "lift_strfix.hpp"

namespace rh {

hipError_t launch_lift_strfix_w16(int vk, int rk, bool tags, const DevCols &c, uint64_t n, uint8_t *fps, uint8_t *bsums,
                                  hipStream_t st) {
    return launch_strfix_width<16>(vk, rk, tags, c, n, fps, bsums, st);
}

}  // namespace rh
