// lift_strfix64.hip -- lift_strfix.hpp instantiated for 64-byte key rows.
#include "lift_strfix.hpp"

namespace rh {

hipError_t launch_lift_strfix_w64(int vk, int rk, bool tags, const DevCols &c, uint64_t n, uint8_t *fps, uint8_t *bsums,
                                  hipStream_t st) {
    return launch_strfix_width<64>(vk, rk, tags, c, n, fps, bsums, st);
}

}  // namespace rh
